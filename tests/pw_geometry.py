"""A plain Python copy of the host arithmetic of csrc/pointwise_kernels.hip: ias_pwconv_supported, pw_vec, pw_apply (forward
and input gradient), ias_pwconv_backward_weight and ias_pwconv_weight_scratch.  Test infrastructure only: the thin 1x1
convolutions' C-ABI tests use it to assert that every shape they name reaches the kernel form it is named for (tiles per
wave, ragged last group, grid-stride loop, chunks per split, empty splits, dead waves, LDS bytes), so a later retuning of
the host code fails those assertions instead of silently moving the shape to another form.  It is tied to the library
through the row count ias_pwconv_backward_weight returns and through ias_pwconv_weight_scratch."""

PW_THREADS, PW_CG, PW_NTI, PW_LDS_FLOATS, PW_WROW, PW_PF = 256, 4, 15, 16384, 65, 8
WAVES = PW_THREADS // 64
GRID_CAP = 1024
LDS_DEFAULT = 64 * 1024      # bytes of dynamic LDS a launch gets without asking for more through the function attribute


def supported(Cin, Cout):
    """ias_pwconv_supported."""
    if Cin <= 0 or Cout <= 0 or Cin & 3 or Cout & 3:
        return 0
    pad_out, pad_in = (Cout + 15) & ~15, (Cin + 15) & ~15
    if pad_out * Cin > PW_LDS_FLOATS or pad_in * Cout > PW_LDS_FLOATS:
        return 0
    return 1 if Cin <= 16 * PW_NTI else 0


def vec(ptr_a, ptr_b, HW):
    """pw_vec: floats per load and store, from the two activation pointers (byte addresses) and HW."""
    bits = ptr_a | ptr_b
    if HW & 3 == 0 and bits & 15 == 0:
        return 4
    if HW & 1 == 0 and bits & 7 == 0:
        return 2
    return 1


def apply_form(B, M, K, HW):
    """pw_apply for y[b] = A x[b], A [M,K] -> dict: T (row tiles of 16), live rows of the last tile, KS (k-steps), cg (tiles
    a wave accumulates), ngroups, last_tiles (tiles of the last group), blocks (of 64 positions), items, grid, looped
    (a wave takes more than one item), lds bytes and whether the launch needs the attribute, rounds (k-steps of each
    prefetch round)."""
    T, blocks, KS = (M + 15) // 16, (HW + 63) // 64, K // 4
    cg = PW_CG
    while cg > 1 and B * blocks * ((T + cg - 1) // cg) < 2048:
        cg -= 1
    ngroups = (T + cg - 1) // cg
    items = B * blocks * ngroups
    grid = min((items + WAVES - 1) // WAVES, GRID_CAP)
    lds = 4 * T * KS * PW_WROW
    return dict(T=T, last_rows=M - 16 * (T - 1), KS=KS, cg=cg, ngroups=ngroups, last_tiles=T - (ngroups - 1) * cg,
                blocks=blocks, items=items, grid=grid, looped=items > grid * WAVES, lds=lds, attribute=lds > LDS_DEFAULT,
                rounds=[min(PW_PF, KS - k) for k in range(0, KS, PW_PF)])


def forward_form(B, Cin, Cout, HW):
    return apply_form(B, Cout, Cin, HW)


def backward_data_form(B, Cin, Cout, HW):
    return apply_form(B, Cin, Cout, HW)


def wgrad_splits(B, Cout, HW):
    T, chunks = (Cout + 15) // 16, (HW + 63) // 64
    return min(max((2048 + B * T - 1) // (B * T), 1), chunks)


def backward_weight_form(B, Cin, Cout, HW, scaled=False):
    """ias_pwconv_backward_weight -> dict: T, NTI, chunks, splits, cps (chunks per split), empty (the splits that lie past
    the last chunk), last_chunks (chunks of the last split that has any), tail (positions of the last chunk), units,
    rows (partial rows = workgroups per row tile: what the entry returns), dead (waves of the last row without a unit),
    grid, lds bytes."""
    T, NTI, chunks = (Cout + 15) // 16, (Cin + 15) // 16, (HW + 63) // 64
    splits = wgrad_splits(B, Cout, HW)
    cps = (chunks + splits - 1) // splits
    empty = [sp for sp in range(splits) if sp * cps >= chunks]
    live = splits - len(empty)
    units = B * splits
    rows = (units + WAVES - 1) // WAVES
    return dict(T=T, NTI=NTI, chunks=chunks, splits=splits, cps=cps, empty=empty, last_chunks=chunks - (live - 1) * cps,
                tail=HW - 64 * (chunks - 1), units=units, rows=rows, dead=rows * WAVES - units, grid=rows * T,
                lds=4 * WAVES * (NTI * 256 + (256 if scaled else 0)))


def weight_scratch_floats(B, Cin, Cout, HW):
    """ias_pwconv_weight_scratch."""
    if B <= 0 or Cin <= 0 or Cout <= 0 or HW <= 0:
        return -1
    return B * wgrad_splits(B, Cout, HW) * Cin * Cout


# ---- the cases of tests/test_pwconv_capi_gpu.py: (B, Cin, Cout, HW) -> what the forward, the input gradient and the weight
# gradient must reach (a subset of each form's dict), and VEC with 16-byte aligned pointers
CASES = [
    # the smallest case: one item, three dead waves in the weight gradient
    ((1, 4, 4, 1), 1, dict(items=1, grid=1, looped=False, T=1, KS=1), dict(items=1), dict(units=1, rows=1, dead=3, cps=1)),
    # M & 15 padding in both orientations
    ((7, 8, 12, 9), 1, dict(T=1, last_rows=12, cg=1), dict(T=1, last_rows=8, cg=1), dict(rows=2, dead=1, cps=1)),
    # 3 chunks, the last holding 2 positions
    ((3, 16, 16, 130), 2, dict(blocks=3, cg=1), dict(blocks=3), dict(chunks=3, splits=3, cps=1, tail=2, empty=[])),
    # more than 64 KB of LDS, through the attribute path
    ((2, 128, 128, 9), 1, dict(lds=66560, attribute=True, cg=1), dict(lds=66560, attribute=True), dict(NTI=8)),
    ((128, 64, 256, 70), 2, dict(T=16, cg=2, ngroups=8, last_tiles=2, lds=66560, attribute=True),
     dict(KS=64, rounds=[8] * 8), dict(splits=1, cps=2, rows=32, dead=0, tail=6)),
    ((65, 72, 72, 2044), 4,
     dict(cg=4, ngroups=2, last_tiles=1, items=4160, grid=1024, looped=True, KS=18, rounds=[8, 8, 2], last_rows=8),
     dict(cg=4, ngroups=2, last_tiles=1, items=4160, grid=1024, looped=True, KS=18, rounds=[8, 8, 2]),
     dict(splits=7, cps=5, last_chunks=2, empty=[], rows=114, dead=1, NTI=5)),
    ((22, 24, 100, 2046), 2, dict(cg=3, T=7, ngroups=3, last_tiles=1, last_rows=4), dict(KS=25, rounds=[8, 8, 8, 1]),
     dict(splits=14, cps=3, empty=[11, 12, 13], last_chunks=2, rows=77, dead=0)),
    ((33, 16, 40, 2047), 1, dict(cg=2, ngroups=2, last_tiles=1, last_rows=8), dict(T=1, cg=1),
     dict(splits=21, cps=2, empty=[16, 17, 18, 19, 20], rows=174, dead=3)),
    ((128, 240, 40, 520), 4, dict(KS=60, T=3), dict(T=15, cg=4, ngroups=4, last_tiles=3, items=4608, grid=1024, looped=True),
     dict(NTI=15, splits=6, cps=2, empty=[5], rows=192, dead=0)),
]
SCALED_WGRAD_LDS = {(128, 240, 40, 520): 65536}      # exactly the 64 KB a launch gets without the attribute
MISALIGNED_SHAPE = (3, 16, 24, 132)                  # HW % 4 == 0: VEC follows the pointers alone


def case_id(case):
    return "x".join(str(v) for v in case[0])


def assert_forms(case):
    """Every named attribute of the three forms equals the transcription's; the shape is one the kernels take."""
    shape, v, fwd, gx, gw = case
    assert supported(shape[1], shape[2]) == 1, shape
    assert vec(0, 0, shape[3]) == v, (shape, vec(0, 0, shape[3]), v)
    for name, want, got in (("forward", fwd, forward_form(*shape)), ("input gradient", gx, backward_data_form(*shape)),
                            ("weight gradient", gw, backward_weight_form(*shape))):
        for k, val in want.items():
            assert got.get(k) == val, (shape, name, k, got.get(k), val)
    if shape in SCALED_WGRAD_LDS:
        assert backward_weight_form(*shape, scaled=True)["lds"] == SCALED_WGRAD_LDS[shape]
    assert weight_scratch_floats(*shape) >= backward_weight_form(*shape)["rows"] * shape[1] * shape[2]
