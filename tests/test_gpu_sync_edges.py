"""GPU: vit_ofdm_sync_dev at the edges of its arithmetic and geometry - the inputs of tests/test_sync_edges_host.py, which
proves on the numpy model that each has the property it is aimed at, through the kernel.  Every comparison is run_sync's:
starts, rot, m^ and tau bit for bit, the six info floats by value, every guard word intact.  No tolerances."""
import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

import test_sync_edges_host as H
from test_gpu_sync import SHAPES, directed, run_sync
from test_sync_host import Params

pytestmark = pytest.mark.gpu


def run_case(V, case, **kw):
    return run_sync(V, case.x, case.prm, case.prs, case.coarse, case.nframes, nco_bits=H.NCO_BITS, **kw)


# ---- 1: planted guard correlations ----------------------------------------------------------------------------------

@pytest.mark.parametrize("nfft", H.PLANT_NFFT)
def test_planted_gammas(V, torch_cuda, nfft):
    """every branch of the arctangent, its boundaries, denormal q and turn, the ties of the rint, one accumulator twice
    and the last level of the tree: the device's gamma words are the planted sums bit for bit - +0 where (-1, -0.0) was
    planted, the accumulators start at +0 - and every other word the model's"""
    case = H.planted_case(nfft)
    dev = {}
    run_case(V, case, device=dev)
    want = np.array([g for _, _, g in case.plan], np.float32) + np.float32(0)  # -0 -> +0
    assert np.array_equal(dev["info"][:, 2:4], want.view(np.uint32))
    t = [name for name, _, _ in case.plan].index("minus one, minus zero")
    assert dev["info"][t, 2:4].tolist() == [0xBF800000, 0]
    run_case(V, case, alias=True, with_info=False)


# ---- 2: the amplitude ladder ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nfft", sorted(H.LADDER_SHAPES))
def test_ladder(V, torch_cuda, nfft):
    """one frame from a largest sample of 2^12 down to 2^-39: the same m^, tau and start down to 2^-34, the denormal
    metric words of the low rungs kept"""
    case = H.ladder_case(nfft)
    dev = {}
    start, rot, info, turn = run_case(V, case, device=dev)
    assert np.array_equal(dev["info"][:, 5], info[:, 5])  # the metric words bit for bit, the denormal ones among them
    high = np.array(case.rungs) >= -34
    assert np.array_equal(start[high], case.true[high])
    metric = info[:, 5].view(np.float32)
    if nfft == 2048:  # no denormal inside the domain: the smallest normal binade on the lowest rung
        assert H.TINY <= metric[-1] < 2 * H.TINY and metric.argmin() == len(metric) - 1
    else:
        assert ((metric > 0) & (metric < H.TINY)).any()


@pytest.mark.parametrize("nfft", sorted(H.LARGEST_SHAPES))
def test_largest_result(V, torch_cuda, nfft):
    """two adjacent carriers of amplitude 2^11: sample magnitudes of 2^12, the header's bound; nothing overflows"""
    info = run_case(V, H.largest_case(nfft))[2]
    assert np.isfinite(info[:, 2:].view(np.float32)).all()


# ---- 3: partial zeros and the threshold -------------------------------------------------------------------------------

def test_window_zero_and_guards_zero(V, torch_cuda):
    case = H.partial_zero_case()
    start, rot, info, turn = run_case(V, case)
    assert info[0, 0].view(np.int32) == -case.prm.M and info[0, 1] == 0 and turn[0] != 0 and turn[1] == 0
    run_case(V, case, alias=True)


def test_wrapped_reference_bins(V, torch_cuda):
    case = H.wrapped_prs_case()
    assert np.array_equal(run_case(V, case)[0], case.true)


def test_strongest_path_at_the_ends_of_the_search(V, torch_cuda):
    case = H.edge_path_case()
    info = run_case(V, case)[2]
    assert info[:, 1].tolist() == [0, 2 * case.prm.W, 2 * case.prm.W]


def test_equal_paths_take_the_first(V, torch_cuda):
    case = H.equal_paths_case()
    info = run_case(V, case)[2]
    assert info[:, 1].tolist() == [3, 8, 3]
    run_case(V, case.with_params(thr=0.5))


@pytest.mark.parametrize("nfft", [64, 256])
@pytest.mark.parametrize("thr", [H.THR_TINY, H.THR_LOW, H.THR_DEEP])
def test_thresholds_in_the_denormal_range(V, torch_cuda, nfft, thr):
    """the ladder with a denormal threshold (the level rounds to 0 or is denormal), 2^-24, and 2^-72 (the level is
    denormal on the low rungs)"""
    run_case(V, H.threshold_case(nfft, thr))


def test_directed_frames_with_the_smallest_threshold(V, torch_cuda):
    """the directed frames of tests/test_gpu_sync.py, the all-zero one among them, with thr = 2^-149 and thr = 1"""
    nfft, G, nsyms, W, M = SHAPES[0]
    x, true, coarse, prs = directed(SHAPES[0])
    for thr in (H.THR_TINY, 1.0):
        run_sync(V, x, Params(nfft, G, nsyms, W, M, thr=thr), prs, coarse, 8)


# ---- 4: the guard loop's geometry -------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(H.GEOMETRY)), ids=["%s-%d-%d-%d" % ((g[3].replace(" ", ""),) + g[0][:2] + (g[0][3],))
                                                            for g in H.GEOMETRY])
def test_guard_loop_geometry(V, torch_cuda, i):
    """Gw == TPB, Gw a divisor of TPB, Gw == 1, Gw > 4 TPB, and totals cp_symbols * Gw on and next to the multiples of
    4 TPB; the coarse table, and aliased by the output on every other call"""
    case = H.geometry_case(i)
    for n, cp in enumerate(case.cps):
        run_case(V, case.with_params(cp_symbols=cp), alias=n % 2 == 1)


# ---- 5: frames outside the domain -------------------------------------------------------------------------------------

def test_frames_outside_the_domain(V, torch_cuda):
    """NaN, Inf and 3e38 frames between good ones: the good frames' words are the model's, every guard word is intact,
    the bad frames' starts are integers of c - W - backoff ... c + W - backoff"""
    case = H.out_of_domain_case()
    start = run_case(V, case, unspecified=case.bad)[0]
    good = [t for t in range(case.nframes) if t not in case.bad]
    assert np.array_equal(start[good] + case.prm.backoff, case.true[good])
