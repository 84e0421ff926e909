"""GPU: vit_ofdm_acquire_dev at the caps and edges of its geometry - the inputs of tests/test_acq_edges_host.py, each run
through run_acq of tests/test_gpu_acq.py: every output word against acquire_model in guarded buffers compared whole, the
samples behind nsamples poisoned.  What each case is for stands with its builder; the partition sizes come from
ACQ_GEOMETRY.

Out of scope, and not forgotten: the second trip of either kernel's grid stride (more than 128 MiB of samples, more than
2^20 periods that hold candidates) - plain strides that carry no state, and far beyond a test of a few seconds."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_acq_edges_host import (BLOCKS, COUNTS, FORMATS, GUARD_NBLK, IQ_F32, TIE_FORMATS, TIE_TARGETS, WINDOWS, as_format,
                                 guard_case, poisoned, power_acq, power_case, power_lg, power_nblks, single_candidate_case,
                                 threshold_case, threshold_pair, tie_case, window_case, with_thr)
from test_acq_host import NONE
from test_gpu_acq import run_acq
from test_iqfmt_host import IQ_CS16, IQ_CU8

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("B", BLOCKS)
def test_every_block_length_in_every_format(V, torch_cuda, B, fmt):
    """the power kernel's cell (B, format): block counts around the wavefront's tile of chunks, from first = 0 and from an
    odd sample, d_power compared in every word, the stream ending in mid-block in front of poisoned samples"""
    geo = V.ACQ_GEOMETRY
    for nblk in power_nblks(power_lg(B, fmt, geo), geo):
        dev, floats, scale, n, j = power_case(B, fmt, nblk)
        for first in (0, 1):
            start, info, p = run_acq(V, dev, floats, fmt, scale, power_acq(B, nblk, first), 2, nsamples=n)
            assert p.size == nblk and (j is None or start[0] != -1)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "%s-%s" % w)
def test_windows_at_their_cap(V, torch_cuda, win, count):
    """Ln, Lr = 4096: a period's candidate count at 1 and around one and two LDS tiles, by Pb (float32) and by the end of
    the stream (CS16); the powers stay in the call's own buffer in the second"""
    geo = V.ACQ_GEOMETRY
    for way, fmt in (("pb", IQ_F32), ("end", IQ_CS16)):
        x, a, nper, k, nk = window_case(win, count, way, geo)
        dev, floats, scale = as_format(x, fmt)
        start, info, _ = run_acq(V, dev, floats, fmt, scale, a, nper, with_power=way == "pb")
        assert start[k] != -1 and info[-1, 0] == NONE


@pytest.mark.parametrize("fmt", TIE_FORMATS)
@pytest.mark.parametrize("d", TIE_TARGETS)
def test_last_minimum_at_a_tile_edge(V, torch_cuda, d, fmt):
    """300 candidates at q = 0, three apart, the last of them the last of an LDS tile, the first of the next and the one
    behind it: the thread that owns it has held an equal q before, in the same tile and in the one before"""
    x, a, nper, k, target = tie_case(d, V.ACQ_GEOMETRY)
    dev, floats, scale = as_format(x, fmt)
    start, info, _ = run_acq(V, dev, floats, fmt, scale, a, nper)
    assert info[k, 0] == target and info[k, 1] == 0 and start[k] == (a.Ln + k * a.Pb + target) * a.B
    run_acq(V, dev, floats, fmt, scale, a, k + 1, with_power=False)  # the period is the call's last: the same words


@pytest.mark.parametrize("fmt", (IQ_F32, IQ_CU8))
def test_period_geometry(V, torch_cuda, fmt):
    """Pb = 1 over 300 periods and two more; a stream of 144, 146 and 147 blocks at Pb = 48 with nperiods = nblk // Pb and
    one and two more than that: the period nblk // Pb holds no candidate, none still, and exactly one"""
    dev, floats, scale, a, k = single_candidate_case(fmt)
    for nper in (300, 302):
        start, info, _ = run_acq(V, dev, floats, fmt, scale, a, nper)
        assert (info[:300, 0] == 0).all() and start[k] != -1
    dev, floats, scale, a = guard_case(fmt)
    for nblk in GUARD_NBLK:
        n = nblk * a.B + 5
        pdev, pfloats = poisoned(dev, floats, fmt, n)
        for nper in (3, 4, 5):
            start, info, p = run_acq(V, pdev, pfloats, fmt, scale, a, nper, with_power=nper != 4, nsamples=n)
            assert p.size == nblk and (info[:3, 0] != NONE).all()
            assert nper == 3 or (info[3, 0] != NONE) == (nblk == GUARD_NBLK[-1])


@pytest.mark.parametrize("fmt", (IQ_F32, IQ_CU8))
def test_threshold_at_equality(V, torch_cuda, fmt):
    """thr equal to a period's q, taken from the model's info word: the start is given; the next float below: -1, and
    the info words are the same"""
    dev, floats, scale, a = threshold_case(fmt)
    at, below = threshold_pair(floats, a)
    s_at, i_at, _ = run_acq(V, dev, floats, fmt, scale, with_thr(a, at), 3)
    s_below, i_below, _ = run_acq(V, dev, floats, fmt, scale, with_thr(a, below), 3, with_power=False)
    assert s_at[1] != -1 and s_below[1] == -1 and np.array_equal(i_at, i_below)
