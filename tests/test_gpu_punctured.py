"""GPU: punctured input (vit_decode_punctured_dev, vit_decode_punctured_varlen_dev) against the numpy depuncturer of
tests/test_punct_host.py followed by the CPU oracle's decoder - bit-exact, every decoded byte."""
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_punct_host import depuncture, fic_segments, keep_mask, puncture

pytestmark = pytest.mark.gpu

TAIL = 6
KERNELS = [0, 1, 2, 3]  # auto, wave-per-frame, packed, latency


def random_segments(rng, framebits, nseg=None):
    """1..8 segments with random lengths (most end mid-period) and random keep masks in which some steps keep all four
    symbols and some none"""
    T = framebits + TAIL
    nseg = min(int(rng.integers(1, 9)) if nseg is None else nseg, T)
    cuts = np.sort(rng.choice(np.arange(1, T), nseg - 1, replace=False)) if nseg > 1 else np.array([], np.int64)
    steps = np.diff(np.concatenate(([0], cuts, [T])))
    segs = []
    for s in steps:
        nibs = rng.integers(0, 16, 8)
        nibs[rng.random(8) < 0.2] = 0    # fully punctured steps
        nibs[rng.random(8) < 0.2] = 15   # nothing punctured
        segs.append((int(s), int(sum(int(v) << (4 * i) for i, v in enumerate(nibs)))))
    return segs


def soft_frames(O, n, framebits, seed):
    """half noisy codewords (3 dB), half uniform bytes"""
    a = O.noisy_frames(n - n // 2, framebits, seed=seed)
    b = O.uniform_symbols((n // 2) * O.sym_len(framebits), seed=seed + 1000).reshape(n // 2, -1)
    return np.concatenate([a, b])


def oracle(O, framebits, punct, segs, erasure, ge=False):
    return O.decode_batch(framebits, depuncture(punct, segs, framebits, erasure), nthreads=8, ge=ge)


def gpu_punctured(V, torch, punct, framebits, n, segs, erasure=128, kernel=0, ge=False, offset=0):
    """decode n frames whose transmitted symbols are punct (n*P bytes) placed `offset` bytes into a buffer that ends
    exactly with them"""
    flat = np.ascontiguousarray(punct, np.uint8).reshape(-1)
    buf = torch.empty(offset + flat.size, dtype=torch.uint8, device="cuda")
    buf[offset:] = torch.from_numpy(flat).cuda()
    d_out = torch.full((n, (framebits + 7) // 8), 0xEE, dtype=torch.uint8, device="cuda")
    old_k, old_ge = V.set_kernel(kernel), V.set_renorm_ge(ge)
    try:
        V.decode_punctured_dev(buf[offset:], d_out, framebits, n, segs, erasure)
        torch.cuda.synchronize()
    finally:
        V.set_kernel(old_k)
        V.set_renorm_ge(old_ge)
    return d_out.cpu().numpy()


@pytest.mark.parametrize("framebits", [768, 2304, 288])
def test_identity_profile_is_the_unpunctured_decode(V, O, torch_cuda, framebits):
    """the all-ones profile (one segment, or several) gives exactly vit_decode_batch_dev's bytes"""
    torch = torch_cuda
    n = 75
    sym = soft_frames(O, n, framebits, seed=framebits)
    for kernel in KERNELS:
        old = V.set_kernel(kernel)
        try:
            d_ref = torch.zeros((n, framebits // 8), dtype=torch.uint8, device="cuda")
            V.decode_batch_dev(torch.from_numpy(sym).cuda(), d_ref, framebits, n)
            torch.cuda.synchronize()
        finally:
            V.set_kernel(old)
        ref = d_ref.cpu().numpy()
        T = framebits + TAIL
        for segs in ([(T, 0xFFFFFFFF)], [(13, 0xFFFFFFFF), (T - 20, 0xFFFFFFFF), (7, 0xFFFFFFFF)]):
            got = gpu_punctured(V, torch, sym, framebits, n, segs, erasure=0, kernel=kernel)
            assert np.array_equal(got, ref), (kernel, segs)


@pytest.mark.parametrize("framebits", [2, 288, 768, 778, 780, 2304, 6912, 9216])
def test_random_profiles(V, O, torch_cuda, framebits):
    """random profiles, every kernel, both comparators; a small batch (latency kernel under auto) and, for auto, one
    of more than 2048 frames (packed kernel) tiled from distinct frames"""
    torch = torch_cuda
    rng = np.random.default_rng(framebits + 11)
    n_small, n_base = 37, 48
    reps = 2048 // n_base + 1
    for ge in (False, True):
        segs = random_segments(rng, framebits)
        P = V.punctured_length(segs, framebits)
        assert P == int(keep_mask(segs, framebits).sum())
        punct = puncture(soft_frames(O, n_small, framebits, seed=framebits + ge), segs, framebits)
        want = oracle(O, framebits, punct, segs, 128, ge=ge)
        for kernel in KERNELS:
            got = gpu_punctured(V, torch, punct, framebits, n_small, segs, kernel=kernel, ge=ge)
            assert np.array_equal(got, want), (framebits, ge, kernel, segs)
        base = puncture(soft_frames(O, n_base, framebits, seed=framebits + 7 + ge), segs, framebits)
        want = oracle(O, framebits, base, segs, 128, ge=ge)
        n = n_base * reps
        assert n > 2048
        for kernel in (0, 2):
            got = gpu_punctured(V, torch, np.tile(base, (reps, 1)), framebits, n, segs, kernel=kernel, ge=ge)
            assert np.array_equal(got.reshape(reps, n_base, -1), np.broadcast_to(want, (reps,) + want.shape)), \
                (framebits, ge, kernel, segs)


@pytest.mark.parametrize("erasure", [0, 127, 128, 255])
def test_erasure_values(V, O, torch_cuda, erasure):
    torch = torch_cuda
    rng = np.random.default_rng(erasure)
    framebits, n = 768, 64
    segs = random_segments(rng, framebits, nseg=4)
    punct = puncture(soft_frames(O, n, framebits, seed=5), segs, framebits)
    want = oracle(O, framebits, punct, segs, erasure)
    if erasure in (0, 255):
        assert not np.array_equal(want, oracle(O, framebits, punct, segs, 128))  # the value matters on this batch
    for kernel in KERNELS:
        assert np.array_equal(gpu_punctured(V, torch, punct, framebits, n, segs, erasure=erasure, kernel=kernel), want)


@pytest.mark.parametrize("framebits", [768, 2, 6912])
def test_odd_offset_odd_length_and_buffer_end(V, O, torch_cuda, framebits):
    """d_punct at an odd byte offset, an odd P, and the last frame's input ending exactly at the end of the
    allocation (a frame's last steps read through the dword load clamped to the frame's end)"""
    torch = torch_cuda
    rng = np.random.default_rng(framebits + 3)
    for _ in range(50):
        segs = random_segments(rng, framebits)
        if V.punctured_length(segs, framebits) % 2 == 1:
            break
    P = V.punctured_length(segs, framebits)
    assert P % 2 == 1
    n = 33
    punct = puncture(soft_frames(O, n, framebits, seed=9), segs, framebits)
    want = oracle(O, framebits, punct, segs, 128)
    for kernel in KERNELS:
        for offset in (1, 3):
            got = gpu_punctured(V, torch, punct, framebits, n, segs, kernel=kernel, offset=offset)
            assert np.array_equal(got, want), (kernel, offset, P)


def test_frames_of_fewer_than_four_transmitted_symbols(V, O, torch_cuda):
    """2-bit frames (8 steps) with P = 0..5: the frames shorter than one dword take byte loads"""
    torch = torch_cuda
    framebits, n = 2, 41
    rng = np.random.default_rng(4)
    sym = soft_frames(O, n, framebits, seed=4)
    for keep in (0x0, 0x1, 0x8000_0100, 0x0040_2001, 0x3000_0003, 0x0101_0101 | 0x0010_0000):
        segs = [(3, keep), (5, keep >> 4)]
        P = V.punctured_length(segs, framebits)
        assert P == int(keep_mask(segs, framebits).sum()) <= 5
        punct = puncture(sym, segs, framebits)
        want = oracle(O, framebits, punct, segs, 128)
        for kernel in KERNELS:
            got = gpu_punctured(V, torch, punct, framebits, n, segs, kernel=kernel, offset=1)
            assert np.array_equal(got, want), (kernel, P)


def test_noise_free_round_trip_fic_shape(V, O, torch_cuda):
    """independent of the oracle's decoder: random bits through the mother code (hard symbols scaled to 0/255),
    FIC-shaped puncturing (every step keeps symbols 0 and 1: the non-catastrophic rate-1/2 code), erasure 128 - the
    decode gives the bits back"""
    torch = torch_cuda
    framebits, n = 768, 96
    rng = np.random.default_rng(12)
    bits = rng.integers(0, 2, (n, framebits), dtype=np.uint8)
    sym = np.stack([O.encode(b) * 255 for b in bits]).astype(np.uint8)
    segs = fic_segments()
    punct = puncture(sym, segs, framebits)
    assert punct.shape == (n, 2304)
    for kernel in KERNELS:
        got = gpu_punctured(V, torch, punct, framebits, n, segs, kernel=kernel)
        assert np.array_equal(np.unpackbits(got, axis=1), bits), kernel


def _varlen_case(V, O, rng, lengths, nframes, ndistinct, seed):
    """a table of nframes descriptors over `lengths` (one profile each, random segments) whose inputs are ndistinct
    punctured frames per length, placed at odd offsets; returns host buffers and the expected output"""
    profiles = [random_segments(rng, fb) for fb in lengths]
    chunks, pos, distinct = [], 1, []  # (profile index, sym_offset, expected bytes)
    for pi, fb in enumerate(lengths):
        punct = puncture(soft_frames(O, ndistinct, fb, seed=seed + fb), profiles[pi], fb)
        want = oracle(O, fb, punct, profiles[pi], 128)
        for j in range(ndistinct):
            chunks.append(punct[j])
            distinct.append((pi, pos, want[j]))
            pos += punct.shape[1]
    sym = np.zeros(pos, np.uint8)
    for (pi, off, _), c in zip(distinct, chunks):
        sym[off:off + c.size] = c
    pick = rng.integers(0, len(distinct), nframes)
    desc = np.zeros(nframes, V.DESC_DTYPE)
    out_sz = np.array([(lengths[distinct[k][0]] + 7) // 8 for k in pick], np.int64)
    desc["out_offset"] = np.concatenate(([0], np.cumsum(out_sz)[:-1]))
    want = np.zeros(int(out_sz.sum()), np.uint8)
    for i, k in enumerate(pick):
        pi, off, w = distinct[k]
        desc["sym_offset"][i], desc["framebits"][i], desc["reserved"][i] = off, lengths[pi], pi
        oo = int(desc["out_offset"][i])
        want[oo:oo + w.size] = w
    return profiles, sym, desc, want


def _run_varlen(V, torch, sym, desc, profiles, max_framebits, out_init, kernel=0, sym_bytes=None, out_bytes=None,
                nprofiles=None, profile_img=None):
    d_sym = torch.from_numpy(sym).cuda()
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    img = V.profiles_bytes(profiles) if profile_img is None else profile_img
    d_prof = torch.from_numpy(img).cuda()
    d_out = torch.from_numpy(out_init.copy()).cuda()
    old = V.set_kernel(kernel)
    try:
        V.decode_punctured_varlen_dev(d_sym, d_out, d_desc, desc.size, max_framebits, d_prof,
                                      len(profiles) if nprofiles is None else nprofiles, sym_bytes=sym_bytes,
                                      out_bytes=out_bytes)
        torch.cuda.synchronize()
    finally:
        V.set_kernel(old)
    assert np.array_equal(d_desc.cpu().numpy(), desc.view(np.uint8))  # the caller's tables are not modified
    assert np.array_equal(d_prof.cpu().numpy(), img)
    return d_out.cpu().numpy()


def test_varlen_config3_like_table(V, O, torch_cuda):
    """32768 frames of 288...6912 bits under 6 profiles (one per length), inputs at odd offsets"""
    torch = torch_cuda
    rng = np.random.default_rng(33)
    lengths = [288, 768, 1536, 2304, 4608, 6912]
    profiles, sym, desc, want = _varlen_case(V, O, rng, lengths, 32768, 8, seed=100)
    got = _run_varlen(V, torch, sym, desc, profiles, 6912, np.full(want.size, 0x5A, np.uint8))
    assert np.array_equal(got, want)
    # a declared maximum above the table's longest frame changes nothing
    got = _run_varlen(V, torch, sym, desc, profiles, 9216, np.full(want.size, 0x5A, np.uint8))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("kernel", KERNELS)
def test_varlen_skips_every_invalid_descriptor(V, O, torch_cuda, kernel):
    """a small table mixing valid frames with every skip reason; the skipped frames' output bytes keep their sentinel.
    Table sizes below and above the device sort's threshold (16 frames)."""
    torch = torch_cuda
    rng = np.random.default_rng(50 + kernel)
    lengths = [288, 768, 3072]
    for nfr in (20, 300):
        profiles, sym, desc, want = _varlen_case(V, O, rng, lengths, nfr, 3, seed=200)
        # extra profiles: [3] nsegs 0, [4] 9 segments, [5] a zero-step segment, [6] steps one short of 768 + 6
        bad = [V.PunctProfile(), V.punct_profile([(86, 0xFFFFFFFF)] * 8), V.punct_profile([(774, 0xFFFFFFFF), (0, 1)]),
               V.punct_profile([(773, 0xFFFFFFFF)])]
        bad[1].nsegs = 9
        img = np.concatenate([V.profiles_bytes(profiles), np.frombuffer(b"".join(bytes(p) for p in bad), np.uint8)])
        sym_bytes, out_bytes = sym.size, want.size
        P = {fb: V.punctured_length(profiles[i], fb) for i, fb in enumerate(lengths)}
        # the frame whose output ends exactly at the end of the output buffer stays valid: it must be decoded
        last = nfr - 1
        assert int(desc["out_offset"][last]) + (int(desc["framebits"][last]) + 7) // 8 == out_bytes
        reasons = [("framebits", 767),            # odd
                   ("framebits", 3074),           # above max_framebits
                   ("reserved", 7),               # profile index >= nprofiles
                   ("profile", 3), ("profile", 4), ("profile", 5), ("profile", 6),  # invalid / not covering 768 + 6
                   ("sym_offset", 1 << 40),       # input far outside
                   ("sym_offset", (1 << 64) - 3),  # offset + P wraps around
                   ("sym_end", None),             # the frame's last input byte lies outside (by one)
                   ("out_offset", 1 << 41),
                   ("out_offset", out_bytes - 1)]  # the frame's last output byte lies outside
        for i, (field, val) in zip(rng.permutation(nfr - 1), reasons):
            fb, oo = int(desc["framebits"][i]), int(desc["out_offset"][i])
            if field == "sym_end":
                desc["sym_offset"][i] = sym_bytes - P[fb] + 1
            elif field == "profile":  # a 768-bit frame under an invalid profile (its output would reach further)
                desc["framebits"][i], desc["reserved"][i] = 768, val
            else:
                desc[field][i] = val
            want[oo:oo + (fb + 7) // 8] = 0x5A  # nothing is written where this frame's bytes would have gone
        got = _run_varlen(V, torch, sym, desc, profiles, 3072, np.full(out_bytes, 0x5A, np.uint8), kernel=kernel,
                          nprofiles=7, profile_img=img)
        assert np.array_equal(got, want), (kernel, nfr)


def test_streams_and_threads_share_the_scratch(V, O, torch_cuda):
    """two threads, each alternating between two streams: punctured batches of different sizes interleaved with
    vit_decode_batch_dev_u32 calls whose unaligned u32 input is narrowed into the same scratch buffer"""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    cases = []
    for fb, n in ((768, 2100), (2304, 61), (6912, 9), (288, 700)):
        segs = random_segments(rng, fb)
        punct = puncture(soft_frames(O, n, fb, seed=fb), segs, fb)
        cases.append((fb, n, segs, torch.from_numpy(punct.reshape(-1)).cuda(), oracle(O, fb, punct, segs, 128)))
    fb32, n32 = 1536, 40
    sym32 = soft_frames(O, n32, fb32, seed=3)
    want32 = O.decode_batch(fb32, sym32, nthreads=8)
    d32 = torch.zeros(sym32.size + 1, dtype=torch.int32, device="cuda")
    d32[1:] = torch.from_numpy(sym32.reshape(-1).astype(np.int32)).cuda()  # 4 bytes in: not 16-byte aligned
    errs = []

    def work(tid):
        try:
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            outs = []
            for rep in range(8):
                st = streams[rep & 1]
                with torch.cuda.stream(st):
                    if rep % 3 == 2:
                        d_out = torch.zeros((n32, fb32 // 8), dtype=torch.uint8, device="cuda")
                        V.decode_batch_dev_u32(d32[1:], d_out, fb32, n32, stream=st.cuda_stream)
                        outs.append((d_out, want32, "u32"))
                    else:
                        fb, n, segs, d_p, want = cases[(tid + rep) % len(cases)]
                        d_out = torch.zeros((n, (fb + 7) // 8), dtype=torch.uint8, device="cuda")
                        V.decode_punctured_dev(d_p, d_out, fb, n, segs, 128, stream=st.cuda_stream)
                        outs.append((d_out, want, fb))
            torch.cuda.synchronize()
            for d_out, want, what in outs:
                if not np.array_equal(d_out.cpu().numpy(), want):
                    errs.append((tid, what))
        except Exception as e:  # noqa: BLE001
            errs.append((tid, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs


def test_full_size_fic_batch(V, O, torch_cuda):
    """65536 FIC-shaped frames (2304 transmitted symbols for 768 bits): 256 distinct frames tiled 256x, every tile
    equal to the oracle's decode of the 256"""
    torch = torch_cuda
    framebits, base_n, reps = 768, 256, 256
    segs = fic_segments()
    base = puncture(soft_frames(O, base_n, framebits, seed=2025), segs, framebits)
    want = oracle(O, framebits, base, segs, 128)
    d_p = torch.from_numpy(base).cuda().repeat(reps, 1).contiguous()
    n = base_n * reps
    d_out = torch.zeros((n, framebits // 8), dtype=torch.uint8, device="cuda")
    V.decode_punctured_dev(d_p, d_out, framebits, n, segs, 128)
    torch.cuda.synchronize()
    assert bool((d_out.view(reps, base_n, -1) == torch.from_numpy(want).cuda().unsqueeze(0)).all())


def test_argument_errors(V, torch_cuda):
    """invalid profiles are VIT_ERR_ARG before anything is launched; empty batches are no-ops"""
    torch = torch_cuda
    d_p = torch.zeros(4 * 774, dtype=torch.uint8, device="cuda")
    d_out = torch.full((1, 96), 0x33, dtype=torch.uint8, device="cuda")
    nine = V.punct_profile([(86, 0xFFFFFFFF)] * 8)
    nine.nsegs = 9
    for segs in ([(773, 0xFFFFFFFF)], [(774, 0xFFFFFFFF), (0, 1)], [(700, 1), (75, 1)], V.PunctProfile(), nine):
        with pytest.raises(V.ViterbiError):
            V.decode_punctured_dev(d_p, d_out, 768, 1, segs)
    with pytest.raises(V.ViterbiError):
        V.decode_punctured_dev(d_p, d_out, 767, 1, [(773, 0xFFFFFFFF)])  # odd framebits
    V.decode_punctured_dev(d_p, d_out, 768, 0, [(1, 1)])  # nframes == 0: OK, nothing checked or touched
    V.decode_punctured_dev(d_p, d_out, 0, 1, [(1, 1)])
    torch.cuda.synchronize()
    assert bool((d_out == 0x33).all())
