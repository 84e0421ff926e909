"""Child process of tests/test_gpu_tb_paths.py::test_diag_counters_equal_the_models: loads the -DVIT_DIAG_SPEC build
(VITERBI_AMD_LIB, set by the parent), decodes every directed batch ONCE with the packed kernels and compares the eight
counters with the totals of tests/tbdirect.py's models and the bytes with the oracle.  Prints one line per batch; exit
status 0 only if everything agrees."""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import _vitpkg  # noqa: E402
import tbdirect as D  # noqa: E402

NAMES = ("groups", "parts_in_flight", "gave_up", "parts_after_forward", "failed_check", "fast_miss0", "fast_passes", "warm90")


def main():
    V = _vitpkg.load_package()
    O = _vitpkg.load_oracle()
    assert os.path.basename(V.LIB_PATH) == "libviterbi_diag.so", V.LIB_PATH
    assert torch.cuda.is_available()
    V.initialize()
    V.set_kernel(2)
    lib = V.lib()
    lib.vit_diag_spec.argtypes = [ctypes.c_void_p, ctypes.c_int]
    waves, _ = D.load_directed()
    bad = 0
    for ge in (False, True):
        V.set_renorm_ge(1 if ge else 0)
        for b in D.batches(waves):
            syms, lens = b.symbols(), b.lengths()
            want = [O.decode_batch(fb, s, ge=ge)[0] for fb, s in zip(lens, syms)]
            model = b.counters(O, ge)
            d_sym = torch.from_numpy(np.concatenate(syms)).cuda()
            d_out = torch.full((sum(w.size for w in want) + 128,), 0xA5, dtype=torch.uint8, device="cuda")
            assert lib.vit_diag_spec(None, 1) == 0
            if b.framebits is not None:
                V.decode_batch_dev(d_sym, d_out[64:], b.framebits, len(lens))
            else:
                desc, _, _ = V.make_descs(lens)
                V.decode_varlen_dev(d_sym, d_out[64:], torch.from_numpy(desc.view(np.uint8)).cuda(), len(lens), max(lens))
            torch.cuda.synchronize()
            c = np.zeros(8, np.uint64)
            assert lib.vit_diag_spec(c.ctypes.data_as(ctypes.c_void_p), 0) == 0
            got = d_out.cpu().numpy()
            ok_bytes = np.array_equal(got[64:-64], np.concatenate(want)) and (got[:64] == 0xA5).all() and (got[-64:] == 0xA5).all()
            ok_c = np.array_equal(c.astype(np.int64), model)
            bad += not (ok_bytes and ok_c)
            print("%s ge=%d %s frames=%d bytes=%s counters=%s model=%s" % (
                "ok  " if ok_bytes and ok_c else "FAIL", ge, b.name, len(lens), ok_bytes,
                dict(zip(NAMES, c.tolist())), model.tolist()), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
