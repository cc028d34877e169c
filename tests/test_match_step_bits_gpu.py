"""The bits of ias_match_adam_step and ias_match_tied_step against a record (tests/golden/match_step_bits.npz, written by
scripts/match_step_bits.py on an MI355X at the commit before the two kernels came to share one Adam update).  The two
kernels are compared with each other in tests/test_tied_gpu.py; this holds both to what shipped."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def test_both_steps_give_the_recorded_bits(lib, dev):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import match_step_bits
    finally:
        sys.path.pop(0)
    want = np.load(os.path.join(GOLDEN, "match_step_bits.npz"))
    got = match_step_bits.replay(dev)
    entries = {("singleton", "adam"): match_step_bits.ARRAYS[:-1], ("singleton", "tied"): match_step_bits.ARRAYS,
               ("groups", "tied"): match_step_bits.ARRAYS}
    assert sorted(got) == sorted(want.files) == sorted(f"{c}_{e}_{k}" for (c, e), ks in entries.items() for k in ks)
    for name in want.files:
        a, b = torch.from_numpy(got[name]), torch.from_numpy(want[name])
        assert a.dtype == b.dtype and torch.equal(a, b), name          # NaN-free by construction: equal means the same bits
    # the record is of runs that did step, skip and take bests
    assert want["singleton_adam_step"].tolist() == [6, 4, 6, 0, 6, 4, 6] and want["groups_tied_step"].tolist() == [5, 5, 0, 5]
    assert want["singleton_tied_skipped"].tolist() == [0, 2, 0, 0, 0, 2, 0]
    assert not np.isnan(want["singleton_adam_params01"]).any() and not np.isnan(want["groups_tied_v"]).any()
