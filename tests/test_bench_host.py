"""CPU checks of bench.py's host logic: the synthetic-input generator follows the reference recipe
(viterbi-benchmark.cpp:293-311) - its noiseless symbols are the oracle encoder's code bits, the payload
hook reproduces given bits - and the sharding arithmetic used for N > 1."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_make_frames_matches_oracle_encoder(O):
    fb, n = 96, 6
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, (n, fb)).astype(np.int32)
    # Eb/N0 = 60 dB: the noise term vanishes, samples saturate at 0 / 255 exactly where the code bit is 0 / 1
    sym = bench.make_frames(n, fb, seed=1, device=torch.device("cpu"), ebn0_db=60.0,
                            payload_bits=torch.from_numpy(bits)).numpy()
    assert sym.shape == (n, 4 * (fb + bench.TAIL)) and sym.dtype == np.uint8
    for i in range(n):
        hard = O.encode(bits[i].astype(np.uint8))
        assert np.array_equal(sym[i] > 127, hard.astype(bool))
        # and the oracle decodes it back (tail-terminated frame)
        assert np.array_equal(np.unpackbits(O.decode_batch(fb, sym[i:i + 1])[0]), bits[i].astype(np.uint8))


def test_make_frames_is_seeded_and_noisy():
    a = bench.make_frames(4, 768, seed=5, device=torch.device("cpu"))
    b = bench.make_frames(4, 768, seed=5, device=torch.device("cpu"))
    c = bench.make_frames(4, 768, seed=6, device=torch.device("cpu"))
    assert torch.equal(a, b) and not torch.equal(a, c)
    v = a.to(torch.float32)
    assert 20 < float(v.std()) < 120 and 0 < int((a == 0).sum()) and 0 < int((a == 255).sum())  # clipped AWGN around 127.5


def test_dump_outputs_samples_a_large_output(tmp_path, monkeypatch):
    """an output above the budget keeps a fixed, seeded sample of its rows, with the row indices next to it"""
    monkeypatch.setattr(bench, "DUMP_BYTES", 100 * 96 * 4)
    out = np.random.default_rng(1).integers(0, 256, (1000, 96), dtype=np.uint8)
    info = bench.dump_outputs(str(tmp_path / "a"), "decoded", out)
    bench.dump_outputs(str(tmp_path / "b"), "decoded", out)
    a, rows = np.load(tmp_path / "a" / "decoded.npy"), np.load(tmp_path / "a" / "decoded_rows.npy")
    assert info["files"] == ["decoded.npy", "decoded_rows.npy"] and a.dtype == np.float32 and rows.dtype == np.float64
    assert a.nbytes + rows.nbytes <= bench.DUMP_BYTES and len(rows) == a.shape[0] > 90
    assert np.array_equal(a, out[rows.astype(np.int64)].astype(np.float32))
    assert np.array_equal(a, np.load(tmp_path / "b" / "decoded.npy"))


def test_bench_constants():
    assert bench.FRAMEBITS == 768 and bench.TAIL == 6 and bench.POLYS == (109, 79, 83, 109)
    assert 4 * (bench.FRAMEBITS + bench.TAIL) + bench.FRAMEBITS // 8 == 3192  # algorithmic bytes per FIC frame
