"""Writes the golden file of tests/test_stft_frame_grad_bits_gpu.py from the library in use (IAS_HIP_LIB or the in-tree one):
   python scripts/diag/make_stft_frame_grad_golden.py OUT.npz
Run it with the library of the commit whose bits are to be kept (the file in tests/golden/ came from the last commit that
held the frame-gradient kernels in csrc/spectral_kernels.hip), on a 256-CU part."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_stft_frame_grad_bits_gpu as T  # noqa: E402


def main(out):
    from inverse_audio_synthesis_amd import _lib
    dev = torch.device("cuda:0")
    lib = _lib.load()
    entries = {"ncu": np.int64(torch.cuda.get_device_properties(0).multi_processor_count)}
    for name in T.CASES:
        grad, plans = T.run_case(name, lib, dev)
        entries[f"{name}/grad"] = grad.numpy()
        entries[f"{name}/plans"] = plans
        print(name, "plans", plans.tolist(), "|grad| max", float(grad.abs().max()), flush=True)
    np.savez_compressed(out, **entries)
    print(out, os.path.getsize(out), "bytes, library", _lib.LIB_PATH)


if __name__ == "__main__":
    main(sys.argv[1])
