"""GPU: one thread's scratch buffers across the entry points that share them - the expansion of vit_decode_punctured_dev,
the narrowing of vit_decode_batch_dev_u32, the checked descriptor copy of vit_decode_varlen_dev_checked and the floats of
vit_ofdm_acquire_dev and vit_ofdm_tii_dev - issued back to back on two streams while the symbol scratch grows."""
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_gpu_acq import make_stream
from test_gpu_ofdm import dev_bins
from test_gpu_ofdm_td import dev_u32, tw_tables
from test_gpu_punctured import oracle, soft_frames
from test_punct_host import fic_segments, puncture

pytestmark = pytest.mark.gpu

SENT64, SENT32 = -0x0123456789ABCDEF, 0x5A5A5A5A
ROUNDS = 12


def tiled(base, n):
    return np.tile(base, ((n + len(base) - 1) // len(base), 1))[:n]


def test_one_thread_scratch_across_entry_points(V, O, torch_cuda):
    """one host thread, two streams, 12 rounds without a synchronisation: acquisition, transmitter identification, the
    checked variable-length decode, the u32 decode under the wave kernel (which never reads u32 in place) and the punctured
    decode in turn, on alternating streams.  The thread is new, so its symbol scratch is allocated by round 0 (64 KiB for
    the acquisition's 146 floats) and grows in round 3 (the 823200 narrowed symbols) while rounds 0 ... 2 are in flight;
    the descriptor scratch is allocated in round 2.  Every output equals that of the same call made alone and
    synchronised, and the decoders' equal the oracle's."""
    torch = torch_cuda
    rng = np.random.default_rng(1717)
    # punctured: FIC profile, 300 frames of 768 bits -> 928800 expanded symbols
    segs = fic_segments()
    base = puncture(soft_frames(O, 64, 768, seed=768), segs, 768)
    d_punct = torch.from_numpy(tiled(base, 300).reshape(-1)).cuda()
    want_punct = tiled(oracle(O, 768, base, segs, 128), 300)
    # u32: 700 frames of 288 bits
    base32 = soft_frames(O, 64, 288, seed=288)
    d_u32 = torch.from_numpy(tiled(base32, 700).reshape(-1).astype(np.int32)).cuda()
    want_u32 = tiled(O.decode_batch(288, base32, nthreads=8), 700)
    # checked varlen: 64 descriptors, every one inside the buffers
    fbs = [int(x) for x in 8 * rng.integers(1, 289, 63)] + [2304]
    desc, sym_bytes, out_bytes = V.make_descs(fbs)
    vsym = O.uniform_symbols(sym_bytes, seed=64)
    want_var = np.zeros(out_bytes, np.uint8)
    for fb, d in zip(fbs, desc):
        so, oo = int(d["sym_offset"]), int(d["out_offset"])
        want_var[oo:oo + fb // 8] = O.decode_batch(fb, vsym[so:so + O.sym_len(fb)])[0]
    d_vsym, d_desc = torch.from_numpy(vsym).cuda(), torch.from_numpy(desc.view(np.uint8)).cuda()
    # acquisition: B = 64 with the geometry of test_gpu_acq's smallest shape, no d_power -> the powers go to the scratch
    B, Ln, Lr, Pb, nper = 64, 2, 1, 48, 3
    d_acq = torch.from_numpy(np.asarray(make_stream((B, Ln, Lr, Pb, nper)), np.complex64)).cuda()
    # transmitter identification: the shape of test_tii_host.argument_error_cases, 4 frames in 2 groups
    nfft, Gp, Cc, R, navg, nfr = 64, 4, 3, 2, 2, 4
    x = (rng.standard_normal(1024) + 1j * rng.standard_normal(1024)).astype(np.complex64)
    d_tiq = torch.from_numpy(x).cuda()
    d_tw = tw_tables(V, nfft)[1]
    d_pairs = dev_bins(2 * np.arange(R * Gp * Cc))
    d_tstart = torch.tensor([100, 300, 500, 700], dtype=torch.int64, device="cuda")
    ngrp = nfr // navg

    def issue(which, st):
        """-> the call's output tensors, allocated and written on stream st"""
        s = st.cuda_stream
        if which == 0:
            so = torch.full((nper,), SENT64, dtype=torch.int64, device="cuda")
            io = dev_u32(np.full(4 * nper, SENT32, np.uint32))
            V.ofdm_acquire_dev(d_acq, B, Ln, Lr, Pb, 4.0, nper, so, offset=B // 2 - 7, d_info=io, stream=s)
            return [so, io]
        if which == 1:
            to = dev_u32(np.full(ngrp * (2 + 2 * Cc), SENT32, np.uint32))
            eo = dev_u32(np.full(ngrp * Gp * Cc, SENT32, np.uint32)).view(torch.float32)
            V.ofdm_tii_dev(d_tiq, nfft, nfr, d_tw, d_pairs, to, Gp, Cc, R, navg, 2.5, -20, d_start=d_tstart, d_energy=eo, stream=s)
            return [to, eo.view(torch.int32)]
        if which == 2:
            out = torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
            V.decode_varlen_dev_checked(d_vsym, out, d_desc, len(fbs), 2304, stream=s)
            return [out]
        if which == 3:
            out = torch.zeros((700, 36), dtype=torch.uint8, device="cuda")
            old = V.set_kernel(1)
            try:
                V.decode_batch_dev_u32(d_u32, out, 288, 700, stream=s)
            finally:
                V.set_kernel(old)
            return [out]
        out = torch.zeros((300, 96), dtype=torch.uint8, device="cuda")
        V.decode_punctured_dev(d_punct, out, 768, 300, segs, 128, stream=s)
        return [out]

    # each call alone, synchronised
    alone = []
    for which in range(5):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            outs = issue(which, st)
        torch.cuda.synchronize()
        alone.append([o.cpu().numpy() for o in outs])
    assert np.array_equal(alone[2][0], want_var), "checked varlen decode, alone"
    assert np.array_equal(alone[3][0], want_u32), "u32 decode, alone"
    assert np.array_equal(alone[4][0], want_punct), "punctured decode, alone"
    assert (alone[0][0] != SENT64).all() and (alone[0][0] != -1).any(), "the acquisition finds nulls"
    assert (alone[1][0] != SENT32).all() and (alone[1][1].view(np.uint32) != SENT32).all(), "every TII word is written"

    errs = []

    def work():
        try:
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            issued = []
            for r in range(ROUNDS):
                st = streams[r & 1]
                with torch.cuda.stream(st):
                    issued.append((r, issue(r % 5, st)))
            torch.cuda.synchronize()
            for r, outs in issued:
                for i, (o, want) in enumerate(zip(outs, alone[r % 5])):
                    if not np.array_equal(o.cpu().numpy(), want):
                        errs.append((r, r % 5, i))
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert not errs, "(round, call, output) that differ from the call made alone: %s" % errs
