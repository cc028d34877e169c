"""Writes the golden file of tests/test_stft2_frame_loop_gpu.py from the library in use (IAS_HIP_LIB or the in-tree one):
   python scripts/diag/make_stft2_frame_loop_golden.py OUT.npz
Run it with the library of the commit whose bits are to be kept (the file in tests/golden/ came from the last commit
whose stft2_kernel held two sets of frame registers), on a 256-CU part."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_stft2_frame_loop_gpu as T  # noqa: E402


def main(out):
    dev = torch.device("cuda:0")
    ncu = T.cu_count()
    entries = {"ncu": np.int64(ncu)}
    for name in T.CASES:
        res = T.run_case(name, dev, ncu)
        entries.update(T.golden_entries(name, res))
        print(name, "B", res["B"], "F", res["F"], flush=True)
    np.savez(out, **entries)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
