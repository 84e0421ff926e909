"""GPU: vit_ofdm_tii_dev at the caps and edges of its geometry - the inputs of tests/test_tii_edges_host.py, each run through
run_tii of tests/test_gpu_tii.py: every word of d_tii and d_energy against tii_model in guarded buffers compared whole, in
float32 and in one integer format per case.  What each case is for stands with its builder; the partition sizes and caps
come from TII_GEOMETRY.

Out of scope, and not forgotten: neither kernel strides over the grid, so a launch has no second trip to test."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_fft_host import F32
from test_gpu_tii import rot_table, run_tii
from test_iqfmt_host import INT_FORMATS
from test_tii_edges_host import (IQ_F32, LAUNCH_SHAPE, NAVG_RUNS, NAVG_SHAPE, SLOT_NFFT, SLOT_SHAPES, THR_ABOVE, THR_AT, TIE_CLASS,
                                 TIE_SHAPES, TINY_SHAPES, as_format, int_format, navg_case, navg_nused, slot_case, tie_case,
                                 tiny_case)
from test_tii_host import Tii, masks_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nfft", SLOT_NFFT)
@pytest.mark.parametrize("shape", SLOT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_slot_counts_around_the_trips(V, torch_cuda, shape, nfft):
    """Gp*C = 255 ... 1024: one to four trips of the group kernel's three loops, every slot of its LDS, bits up to 31 of a
    mask; three frames in groups of two, float32 with the rotation and an integer format without"""
    Gp, C_ = shape
    x, starts, offset, pairs, R, on, off = slot_case(nfft, Gp, C_)
    p = Tii(nfft, Gp, C_, R, navg=2, thr=2.5, offset=offset)
    case = SLOT_SHAPES.index(shape) + SLOT_NFFT.index(nfft)
    for fmt, rot in ((IQ_F32, rot_table(np.random.default_rng(case), 3)), (int_format(case), None)):
        samples, mfmt = as_format(x, fmt)
        words, _ = run_tii(V, samples, mfmt, p, pairs, 3, starts=starts, rot=rot)
        assert words[:, 0].tolist() == [2, 1] and masks_of(words).any()


@pytest.mark.parametrize("navg,nframes", NAVG_RUNS)
def test_navg_at_its_cap(V, torch_cuda, navg, nframes):
    """255 and 256 frames per estimate, skipped frames at both ends of a group's list, a ragged group of one"""
    nfft, Gp, C_, R = NAVG_SHAPE
    x, starts, offset, pairs, on, off = navg_case()
    p = Tii(nfft, Gp, C_, R, navg=navg, thr=2.5, offset=offset)
    case = NAVG_RUNS.index((navg, nframes))
    for fmt in (IQ_F32, int_format(case)):
        samples, mfmt = as_format(x, fmt)
        words, _ = run_tii(V, samples, mfmt, p, pairs, nframes, starts=starts, with_energy=fmt == IQ_F32)
        assert words[:, 0].tolist() == navg_nused(navg, nframes)


@pytest.mark.parametrize("shape", TINY_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_odd_and_tiny_slot_counts(V, torch_cuda, shape):
    """1, 3 and 15 slots, 8 repetitions: the median of an odd count, and of one"""
    Gp, C_, R = shape
    x, starts, offset, pairs, on = tiny_case(*shape)
    case = TINY_SHAPES.index(shape)
    for fmt in (IQ_F32, int_format(case)):
        samples, mfmt = as_format(x, fmt)
        for thr in (1.0, 2.5):
            words, energy = run_tii(V, samples, mfmt, Tii(64, Gp, C_, R, navg=2, thr=thr, offset=offset), pairs, 3, starts=starts,
                                    rot=rot_table(np.random.default_rng(case), 3) if thr == 2.5 else None)
            if Gp * C_ == 1:
                assert np.array_equal(words[:, 1].view(F32), energy.reshape(-1))


@pytest.mark.parametrize("shape", TIE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_ties_at_the_median_and_the_threshold(V, torch_cuda, shape):
    """four slots equal the noise level bit for bit, the wanted rank held by one with equal slots on either side of it
    (group 0) and by the last of them (group 1): at thr 1.0 their bits are set, at the next float clear"""
    Gp, C_ = shape
    x, starts, offset, pairs = tie_case(Gp, C_)
    for fmt in (IQ_F32,) + INT_FORMATS:
        samples, mfmt = as_format(x, fmt)
        at = run_tii(V, samples, mfmt, Tii(64, Gp, C_, 1, navg=1, thr=THR_AT, offset=offset), pairs, 2, starts=starts)[0]
        above = run_tii(V, samples, mfmt, Tii(64, Gp, C_, 1, navg=1, thr=THR_ABOVE, offset=offset), pairs, 2, starts=starts)[0]
        for s in TIE_CLASS:
            assert (masks_of(at)[:, s % C_] >> (s // C_) & 1).all() and not (masks_of(above)[:, s % C_] >> (s // C_) & 1).any()
        assert np.array_equal(at[:, :2], above[:, :2])


def test_a_group_does_not_depend_on_nframes_at_1024_slots(V, torch_cuda):
    """one frame, and five frames in groups of one: group 0 has the same words and energies"""
    nfft, Gp, C_ = LAUNCH_SHAPE
    x, starts, offset, pairs, R, on, off = slot_case(nfft, Gp, C_, nframes=5)
    p = Tii(nfft, Gp, C_, R, navg=1, thr=2.5, offset=offset)
    for fmt in (IQ_F32, int_format(2)):
        samples, mfmt = as_format(x, fmt)
        w5, e5 = run_tii(V, samples, mfmt, p, pairs, 5, starts=starts)
        w1, e1 = run_tii(V, samples, mfmt, p, pairs, 1, starts=starts)
        assert np.array_equal(w5[:1], w1) and np.array_equal(e5[:1].view(np.uint32), e1.view(np.uint32))
