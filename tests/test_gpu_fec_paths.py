"""GPU: vit_packet_fec_dev on the syndrome-directed rows of tests/fecdirect.py - every decoder path the classifier
names, at every row and every frame position of a workgroup, at every 16-byte phase of the image, and in bulk on rows
beyond the code's reach.  Bytes and records against decode_row_model (fecdirect.RowModel), byte for byte; every case in
place and out of place with sentinel bytes on both sides (run_fec of tests/test_gpu_packet.py)."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

import fecdirect as fd
from test_gpu_packet import FEC_FPB, run_fec
from test_packet_host import FEC_FRAME_BYTES, FEC_REC_DTYPE, IDX, NCODE, ROWS, SLOT, same

pytestmark = pytest.mark.gpu

FPW = FEC_FPB // 4  # frames per wavefront


@pytest.fixture(scope="module")
def model():
    return fd.RowModel()


def check(V, torch, model, frames, phase=0, off_in=0, off_out=0, head=0, tail=0, seed=0):
    """frames (F, 2472) behind `head` and in front of `tail` slots of other bytes: device == model"""
    rng = np.random.default_rng(seed)
    frames = np.asarray(frames, np.uint8).reshape(-1, FEC_FRAME_BYTES)
    want, wrec = model.frames(frames)
    a, b = rng.integers(0, 256, SLOT * head, dtype=np.uint8), rng.integers(0, 256, SLOT * tail, dtype=np.uint8)
    got, rec = run_fec(V, torch, np.concatenate([a, frames.reshape(-1), b]), phase, off_in, off_out)
    assert len(rec) == len(wrec) and same(rec, wrec), [(int(f), rec[f], wrec[f]) for f in np.flatnonzero(rec != wrec)[:4]]
    wantst = np.concatenate([a, want.reshape(-1), b])
    assert np.array_equal(got, wantst), np.flatnonzero(got != wantst)[:8]
    return wrec


def test_fec_whole_directed_set(V, torch_cuda, model):
    rng = np.random.default_rng(21)
    D = fd.directed_set()
    n = -(-len(D) // ROWS)
    rows = fd.clean_rows(rng, n * ROWS)
    for k, e in enumerate(D):
        rows[k] = e.row
    wrec = check(V, torch_cuda, model, fd.frames_of_rows(rows.reshape(n, ROWS, NCODE)))
    assert wrec["nerr"].reshape(-1)[:len(D)].tolist() == [e.nerr for e in D]
    # and every row alone in its wavefront's company of clean rows, the set in another order
    order = rng.permutation(len(D))
    rows = fd.clean_rows(rng, -(-len(D) // 4) * ROWS).reshape(-1, ROWS, NCODE)  # four directed rows a frame
    for k, j in enumerate(order):
        rows[k // 4, (3 * (k % 4) + k // 4) % ROWS] = D[j].row
    wrec = check(V, torch_cuda, model, fd.frames_of_rows(rows), off_in=1, off_out=1)
    assert sorted(wrec["nerr"][wrec["nerr"] != 0].tolist()) == sorted(e.nerr for e in D)


def test_fec_every_path_at_every_row_and_frame_position(V, torch_cuda, model):
    rng = np.random.default_rng(22)
    reps = fd.representatives()
    groups = list(fd.GROUPS)
    per_wg = 6  # groups per workgroup: six damaged rows a frame, the others clean
    nwg = -(-len(groups) // per_wg)
    rows = fd.clean_rows(rng, (nwg + 4) * FEC_FPB * ROWS).reshape(-1, ROWS, NCODE)
    placed = []  # (group, workgroup, frame position, row)
    for gi, g in enumerate(groups):
        wg = gi // per_wg
        for pos in range(FEC_FPB):
            r = (pos + 2 * (gi % per_wg) + wg) % ROWS
            rows[wg * FEC_FPB + pos, r] = reps[g].row
            placed.append((g, wg, pos, r))
    cells = {(w, p, r) for _, w, p, r in placed}
    assert len(cells) == len(placed), "no placement overwrites another"
    for g in groups:
        assert {r for x, _, _, r in placed if x == g} == set(range(ROWS)), g
        assert {p for x, _, p, _ in placed if x == g} == set(range(FEC_FPB)), g
    lanes = {(p % FPW) * ROWS + r for _, _, p, r in placed}
    assert lanes == set(range(FPW * ROWS)), "every lane 0 ... 59 owns a damaged row somewhere"
    # a wavefront with all 60 rows to correct, and one whose only damaged row is lane 59
    good = [e for e in fd.directed_set() if e.nerr > 0 and e.group != "single"]
    wg = nwg
    for k in range(FPW * ROWS):
        rows[wg * FEC_FPB + FPW + k // ROWS, k % ROWS] = good[(7 * k) % len(good)].row  # wavefront 1
    rows[wg * FEC_FPB + 3 * FPW + FPW - 1, ROWS - 1] = reps["lam_zero"].row  # wavefront 3, frame 4, row 11
    # a workgroup whose damaged rows are all beyond correction (in place it writes nothing) between two that correct
    wg = nwg + 1
    rows[wg * FEC_FPB + 2, 5] = reps["single"].row
    wg = nwg + 2
    fails = [e for e in fd.directed_set() if e.nerr < 0]
    for k, e in enumerate(fails):
        rows[wg * FEC_FPB + (k * 7) % FEC_FPB, (k * 5 + k // 12) % ROWS] = e.row
    wg = nwg + 3
    rows[wg * FEC_FPB + 19, 0] = reps["seam"].row
    frames = fd.frames_of_rows(rows)
    wrec = check(V, torch_cuda, model, frames, phase=1, head=1, tail=2, off_in=3, off_out=3)
    assert wrec["nerr"][nwg * FEC_FPB + FPW:nwg * FEC_FPB + 2 * FPW].min() >= 2
    lone = wrec["nerr"][nwg * FEC_FPB + 3 * FPW:nwg * FEC_FPB + 4 * FPW]
    assert lone[FPW - 1, ROWS - 1] == 8 and int((lone != 0).sum()) == 1
    allbad = wrec["nerr"][(nwg + 2) * FEC_FPB:(nwg + 3) * FEC_FPB]
    assert int((allbad < 0).sum()) == len(fails) >= 40 and not (allbad > 0).any(), "no row of that workgroup is corrected"
    for g, w, p, r in placed:
        assert wrec["nerr"][w * FEC_FPB + p, r] == reps[g].nerr


def test_fec_every_image_phase(V, torch_cuda, model):
    rng = np.random.default_rng(23)
    D = fd.directed_set()
    pick = [e for e in D if e.group != "single"]
    rows = np.stack([pick[(5 * k) % len(pick)].row for k in range(2 * ROWS)]).reshape(2, ROWS, NCODE)
    frames = fd.frames_of_rows(rows)
    frames[1, -5:] = rng.integers(1, 256, 5, dtype=np.uint8)
    seen = set()
    for a in range(16):  # the image's phase: the address of the first frame mod 16
        phase = a % 3
        off = (a - SLOT * phase) % 16  # 24 * phase mod 16 is 0 or 8
        seen.add((off + SLOT * phase) % 16)
        for off_out in (off, (off + 5) % 16):  # d_out at the same phase in 16 bytes, and at another
            check(V, torch_cuda, model, frames, phase=phase, off_in=off, off_out=off_out, head=phase, tail=off % 2, seed=off)
    assert seen == set(range(16))


def test_fec_bulk_beyond_reach(V, torch_cuda):
    """every row of 240 frames carries 9 ... 20 errors or random bytes: against the host twin (which
    tests/test_fec_paths_host.py holds against the model), and 200 sampled rows against the model itself"""
    rng = np.random.default_rng(24)
    F = 12 * FEC_FPB
    heavy = fd.heavy_rows(rng, F * ROWS)
    frames = fd.frames_of_rows(heavy.reshape(F, ROWS, NCODE))
    want = np.empty_like(frames)
    wrec = np.zeros(F, FEC_REC_DTYPE)
    for f in range(F):
        want[f], wrec[f] = V.packet_fec_frame_host(frames[f])
    got, rec = run_fec(V, torch_cuda, frames.reshape(-1), 0, 2, 7)
    assert same(rec, wrec), np.flatnonzero(rec != wrec)[:8]
    assert np.array_equal(got, want.reshape(-1)), np.flatnonzero(got != want.reshape(-1))[:8]
    outcomes = set()
    for k in rng.permutation(F * ROWS)[:200]:
        f, r = divmod(int(k), ROWS)
        row, ne = fd.decode_row_model(frames[f, IDX[r]])
        assert rec["nerr"][f, r] == ne and np.array_equal(got.reshape(F, -1)[f, IDX[r]], row), (f, r, ne)
        outcomes.add(ne)
    assert -1 in outcomes
