"""A plain Python copy of the host geometry of csrc/conv_kernels.hip: dw_wave_geometry, dw_tile_geometry, dw_wave_grid, the
`bch` loop of ias_dwconv_backward_weight, the stride-2 input gradient's choice and the stem's choice of forms.  Test
infrastructure only: the depthwise and stem C-ABI tests use it to assert that every shape they name reaches the kernel
form it is named for, so a later retuning of the host code fails those assertions instead of silently moving the shape
to another form.  It is tied to the library through the row count ias_dwconv_backward_weight returns."""

CV_THREADS, DW_MAX_TILES, DWW_NL, DWW_NI = 256, 8, 16, 4
LDS_LIMIT = 65536           # bytes of dynamic LDS a launch may ask for: the entries refuse a tile geometry above it
WAVE_LDS, CU_LDS, CUS, WAVES_PER_CU = 10240, 160 * 1024, 256, 32


def _cdiv(a, b):
    """C's integer division (towards zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def out_size(n, K, S):
    return _cdiv(n + 2 * ((K - 1) // 2) - K, S) + 1


def _padded_width(W, Wo, K, S):
    P, quads, nseg4 = (K - 1) // 2, (Wo + 3) // 4, (3 * S + K + 3) // 4
    return (max(W + 2 * P, (quads - 1) * 4 * S + 4 * nseg4) + 3) & ~3


def wave_geometry(B, H, W, Ho, Wo, K, S):
    """dw_wave_geometry -> dict (PW, tpp, Wp, rows_in, nl, ni, bch, ntiles, rt, lds), or None where the C code returns
    ok = false (the plane goes to dw_tile_kernel)."""
    quads, HW = (Wo + 3) // 4, H * W
    g = dict(Wp=_padded_width(W, Wo, K, S), bch=min(B, 8), ntiles=1, rt=Ho)
    nitems = Ho * quads
    if HW <= 64 * DWW_NL and nitems <= 64 * DWW_NI:
        tpp = 16 if nitems <= 16 else 32 if nitems <= 32 else 64
        while tpp < 64 and (64 // tpp) * HW > 64 * DWW_NL:
            tpp *= 2
        g.update(tpp=tpp, PW=64 // tpp, rows_in=(Ho - 1) * S + K)
        g["nl"] = (g["PW"] * HW + 63) // 64
    else:
        if quads > 64:
            return None
        rt = 64 // quads
        while rt > 1 and ((rt - 1) * S + K) * W > 64 * DWW_NL:
            rt -= 1
        if ((rt - 1) * S + K) * W > 64 * DWW_NL:
            return None
        g.update(rt=rt, ntiles=(Ho + rt - 1) // rt)
        if g["ntiles"] < 2:
            return None
        g.update(tpp=64, PW=1, rows_in=(rt - 1) * S + K)
        if g["rows_in"] > H:
            return None
        g["nl"] = (g["rows_in"] * W + 63) // 64
        nitems = rt * quads
    g["ni"] = (nitems + g["tpp"] - 1) // g["tpp"]
    g["lds"] = 4 * (g["PW"] * g["rows_in"] * g["Wp"] + g["PW"] * K * K + 4)
    if not (g["nl"] <= DWW_NL and g["ni"] <= DWW_NI and g["lds"] <= WAVE_LDS):
        return None
    g["form"] = (4, 1) if g["nl"] <= 4 and g["ni"] <= 1 else (16, 1) if g["ni"] <= 1 else (16, 4)   # template <NL, NI>
    return g


def wave_grid(g, nwork):
    per_cu = max(1, min(WAVES_PER_CU, CU_LDS // max(g["lds"], 1)))
    return min(nwork, CUS * per_cu)


def tile_geometry(H, W, Ho, Wo, K, S, mode):
    """dw_tile_geometry -> dict (pp, rows_out, Wp, ntiles, lds, walks); `walks`: more than DW_MAX_TILES row tiles, which one
    workgroup per plane then walks itself."""
    Wp, budget = _padded_width(W, Wo, K, S), 8192
    quads, rows_full = (Wo + 3) // 4, (Ho - 1) * S + K
    if rows_full * Wp <= budget:
        pp = 1
        while pp * 2 <= 64 and pp * 2 * rows_full * Wp <= budget and pp * 2 * Ho * quads <= CV_THREADS:
            pp *= 2
        ro = Ho
    else:
        pp = 1
        ro = max(1, _cdiv(budget // 2 // Wp - K, S) + 1)
        if (Ho + ro - 1) // ro > DW_MAX_TILES:
            ro = (Ho + DW_MAX_TILES - 1) // DW_MAX_TILES
        if ((ro - 1) * S + K) * Wp > budget:
            ro = max(1, _cdiv(budget // Wp - K, S) + 1)
    ntiles = (Ho + ro - 1) // ro
    walks = ntiles > DW_MAX_TILES
    if walks:
        ntiles = 1
    rows_in = (ro - 1) * S + K
    lds = 4 * (pp * rows_in * Wp + (CV_THREADS * K * K if mode == 1 else pp * K * K))
    return dict(pp=pp, rows_out=ro, Wp=Wp, ntiles=ntiles, lds=lds, walks=walks, row_tiled=rows_full * Wp > budget)


def _conv_form(B, C, H, W, Ho, Wo, K, S):
    """The form ias_dwconv_forward takes for x [B,C,H,W] -> [.,.,Ho,Wo] (and the stride-1 input gradient with H, W the
    cotangent's extents)."""
    planes = B * C
    g = wave_geometry(B, H, W, Ho, Wo, K, S)
    if g is not None and planes >= g["PW"]:
        nwork = planes * g["ntiles"] if g["ntiles"] > 1 else (planes + g["PW"] - 1) // g["PW"]
        grid = wave_grid(g, nwork)
        return dict(g, kind="wave", nwork=nwork, grid=grid, looped=nwork > grid,
                    moved_back=g["ntiles"] == 1 and planes % g["PW"] != 0)
    t = tile_geometry(H, W, Ho, Wo, K, S, 0)
    return dict(t, kind="tile", refused=t["lds"] > LDS_LIMIT)


def forward_form(B, C, H, W, K, S):
    return _conv_form(B, C, H, W, out_size(H, K, S), out_size(W, K, S), K, S)


def backward_data_form(B, C, H, W, K, S):
    Ho, Wo = out_size(H, K, S), out_size(W, K, S)
    if S == 1:
        return _conv_form(B, C, Ho, Wo, H, W, K, 1)
    if (Ho + 2) * (Wo + 2) <= 12288:
        plane, pp = (Ho + 2) * (Wo + 2), 1
        while pp * 2 <= 64 and pp * 2 * plane <= 8192 and pp * 2 * Ho * Wo <= CV_THREADS:
            pp *= 2
        return dict(kind="s2tile", pp=pp, lds=4 * (pp * plane + pp * K * K))
    return dict(kind="direct")


def backward_weight_form(B, C, H, W, K, S):
    """The form ias_dwconv_backward_weight takes, with `rows`, the number of partial rows it leaves and returns."""
    Ho, Wo = out_size(H, K, S), out_size(W, K, S)
    g = wave_geometry(B, H, W, Ho, Wo, K, S)
    if g is not None and C >= g["PW"]:
        cgroups, bch = (C + g["PW"] - 1) // g["PW"], g["bch"]
        while bch > 1 and cgroups * ((B + bch - 1) // bch) < 2048:
            bch >>= 1
        nchunk = (B + bch - 1) // bch
        nwork = cgroups * nchunk
        grid = wave_grid(g, nwork)
        return dict(g, kind="wave", bch=bch, nchunk=nchunk, rows=nchunk, nwork=nwork, grid=grid, looped=nwork > grid,
                    ragged=B % bch != 0, moved_back=C % g["PW"] != 0, nsteps=bch * g["ntiles"])
    t = tile_geometry(H, W, Ho, Wo, K, S, 1)
    return dict(t, kind="tile", rows=B * t["ntiles"], refused=t["lds"] > LDS_LIMIT)


def weight_scratch_floats(B, C, H, W, K, S):
    return B * C * K * K * tile_geometry(H, W, out_size(H, K, S), out_size(W, K, S), K, S, 1)["ntiles"]


def stem_forms(B, H, W):
    """ias_stem_forward / ias_stem_backward_weight of the product library -> (forward form, chunks of the staged forward,
    weight-gradient form, its partial rows)."""
    Ho, Wo = out_size(H, 3, 2), out_size(W, 3, 2)

    def stride(gw, mod):
        xs = max(2 * gw + 2, W + 2)
        while xs % 32 != mod:
            xs += 1
        return xs
    if 3 * H * W > 0x7fffffff:
        fwd = "valu"
    else:
        fwd = "stage" if stride((Wo + 31) // 32 * 32, 3) <= 320 else "gather"
    chunks = 60 if Ho >= 60 else 1
    gw64 = (Wo + 63) // 64 * 64
    xs, gs = stride(gw64, 3), gw64
    while gs % 32 != 1:
        gs += 1
    staged = gw64 == 128 and xs <= 320 and 2 * (9 * xs + 16 * gs) * 4 <= 65536
    return dict(fwd=fwd, chunks=chunks, gw="stage" if staged else "gather", rows=B * (16 if staged else 32), Ho=Ho, Wo=Wo)


# ---- the depthwise cases of tests/test_dwconv_capi_gpu.py: (B, C, H, W, K, S) -> what the forward, the weight gradient and
# the input gradient must reach (a subset of the form's dict; asserted against the functions above)
W41, W161, W164 = (4, 1), (16, 1), (16, 4)
SMALL_CASES = [
    ((3, 5, 4, 4, 3, 1), dict(kind="wave", form=W41, PW=4, moved_back=True), dict(kind="wave"), dict(kind="wave")),
    ((1, 3, 8, 8, 3, 1), dict(kind="tile", pp=16), dict(kind="tile"), dict(kind="tile")),
    ((2, 3, 2, 1, 5, 2), dict(kind="wave"), dict(kind="tile"), dict(kind="s2tile")),
    ((2, 3, 15, 16, 5, 1), dict(kind="wave", form=W41, PW=1), dict(kind="wave"), dict(kind="wave")),
    ((2, 3, 15, 16, 5, 2), dict(kind="wave", form=W161, PW=4), dict(kind="tile"), dict(kind="s2tile", pp=4)),
    ((2, 3, 30, 31, 3, 1), dict(kind="wave", form=W164), dict(kind="wave"), dict(kind="wave")),
    ((1, 1, 64, 16, 3, 1), dict(kind="wave", form=W164, ntiles=1), dict(kind="wave"), dict(kind="wave")),
    ((1, 1, 65, 16, 5, 1), dict(kind="wave", ntiles=5), dict(kind="wave", nsteps=5), dict(kind="wave", ntiles=5)),
    ((2, 2, 40, 37, 5, 2), dict(kind="wave", ntiles=2, nl=16), dict(kind="wave"), dict(kind="s2tile")),
    ((1, 1, 1, 1, 3, 1), dict(kind="tile", pp=64), dict(kind="tile"), dict(kind="tile")),
    ((1, 1, 1, 1, 5, 2), dict(kind="tile", pp=64), dict(kind="tile"), dict(kind="s2tile")),
    ((1, 2, 1, 70, 3, 2), dict(kind="tile"), dict(kind="tile"), dict(kind="s2tile")),
    ((1, 2, 20, 300, 5, 2), dict(kind="tile", row_tiled=False, pp=1), dict(kind="tile"), dict(kind="s2tile")),
    ((1, 1, 40, 261, 5, 1), dict(kind="tile", ntiles=4, walks=False), dict(kind="tile", rows=4), dict(kind="tile")),
    ((1, 1, 9, 1700, 5, 1), dict(kind="tile", walks=True), dict(kind="tile", walks=True), dict(kind="tile", walks=True)),
    ((1, 1, 300, 200, 3, 2), dict(kind="wave", ntiles=75), dict(kind="wave", nsteps=75), dict(kind="direct")),
]
_LOOP = dict(kind="wave", looped=True)
LOOPED_CASES = [
    ((129, 257, 8, 8, 5, 1), dict(_LOOP, form=W41, PW=4, nwork=8289, moved_back=True),
     dict(kind="wave", bch=4, nchunk=33, ragged=True), dict(_LOOP, nwork=8289, moved_back=True)),
    ((129, 257, 8, 8, 3, 2), dict(_LOOP, form=W41, PW=4, nwork=8289, moved_back=True),
     dict(kind="wave", bch=4, nchunk=33, ragged=True), dict(kind="s2tile")),
    ((3, 391, 40, 37, 3, 1), dict(_LOOP, ntiles=7, nwork=8211), dict(kind="wave", bch=1), dict(_LOOP, ntiles=7)),
    ((2, 821, 65, 16, 5, 1), dict(_LOOP, ntiles=5, nwork=8210), dict(kind="wave", bch=1), dict(_LOOP, ntiles=5)),
    ((1, 1640, 150, 30, 5, 2), dict(_LOOP, ntiles=5, nwork=8200), dict(kind="wave", bch=1), dict(kind="s2tile")),
    ((9, 911, 30, 31, 3, 1), dict(_LOOP, form=W164, ntiles=1, nwork=8199), dict(kind="wave", bch=4, ragged=True),
     dict(_LOOP, form=W164)),
    ((65, 4101, 4, 4, 3, 1), dict(_LOOP), dict(_LOOP, bch=8, nchunk=9, ragged=True, moved_back=True), dict(_LOOP)),
    ((13, 1024, 15, 16, 5, 1), dict(_LOOP), dict(kind="wave", bch=8, nchunk=2, ragged=True), dict(_LOOP)),
    ((17, 1024, 4, 4, 3, 1), dict(kind="wave", looped=False), dict(kind="wave", bch=2, ragged=True), dict(kind="wave")),
    ((5, 1024, 33, 31, 3, 1), dict(_LOOP, ntiles=5), dict(kind="wave", ntiles=5, bch=2, ragged=True), dict(_LOOP, ntiles=5)),
    ((3, 2048, 40, 37, 5, 2), dict(_LOOP, ntiles=2), dict(kind="wave", bch=3, ragged=False), dict(kind="s2tile")),
]
LDS_CASE = ((1, 1, 3, 2100, 5, 1), dict(kind="tile", lds=42180, refused=False), dict(kind="tile", lds=67680, refused=True),
            dict(kind="tile", refused=False))
CASES = SMALL_CASES + LOOPED_CASES


def case_id(case):
    return "x".join(str(v) for v in case[0])


def assert_forms(case):
    """Every named attribute of the three forms equals the transcription's."""
    shape, fwd, gw, gx = case
    for name, want, got in (("forward", fwd, forward_form(*shape)), ("weight gradient", gw, backward_weight_form(*shape)),
                            ("input gradient", gx, backward_data_form(*shape))):
        for k, v in want.items():
            assert got.get(k) == v, (shape, name, k, got.get(k), v)
    assert weight_scratch_floats(*shape) >= backward_weight_form(*shape)["rows"] * shape[1] * shape[4] ** 2


# ---- the stem cases of tests/test_stem_capi_gpu.py: (B, H, W) -> what stem_forms must give
STEM_CASES = [
    ((2, 1, 1), dict(fwd="stage", gw="gather")),
    ((3, 2, 2), dict(fwd="stage", gw="gather")),
    ((3, 17, 10), dict(fwd="stage", gw="gather")),
    ((2, 7, 129), dict(Wo=65, fwd="stage", gw="stage")),
    ((2, 5, 255), dict(Wo=128, fwd="stage", gw="stage")),
    ((2, 5, 256), dict(Wo=128, fwd="stage", gw="stage")),
    ((2, 5, 257), dict(Wo=129, fwd="gather", gw="gather")),
    ((1, 118, 9), dict(Ho=59, chunks=1)),
    ((1, 119, 9), dict(Ho=60, chunks=60)),
    ((1, 121, 9), dict(Ho=61, chunks=60)),
    ((3, 33, 130), dict(Ho=17, gw="stage")),
    ((1, 65, 9), dict(Ho=33, gw="gather")),
    ((5, 121, 128), dict(Wo=64, gw="gather")),
]
