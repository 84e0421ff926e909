"""GPU: after the decoder - energy dispersal (vit_energy_dispersal_dev / _varlen_dev), the FIB CRC (vit_fib_crc_dev),
the FIC chain (vit_decode_fic_dev) and the DAB+ chain (vit_dabplus_punctured_superframes_dev) - against the models of
tests/test_dab_host.py, the numpy depuncturer of tests/test_punct_host.py and the CPU oracle's decoder and RS check."""
import os
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_dab_host import fib_ok_model, fire_ok_model, make_fib, scramble, with_fire_code
from test_punct_host import KEEP_24, KEEP_TAIL_12, depuncture, fic_segments, puncture

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import rs_encode_columns  # noqa: E402

pytestmark = pytest.mark.gpu

TAIL = 6
GUARD = 16


# ---- inputs ---------------------------------------------------------------------------------------------------------

def channel(O, frames, framebits, rng, mode):
    """(n, (framebits+7)//8) bytes -> (n, 4*(framebits+6)) u8 symbols through the mother code.  mode: 'clean' (0/255),
    '3dB' (soft, AWGN at Eb/N0 = 3 dB for the rate-1/4 mother code), 'flip' (hard, 8 % of the symbols inverted),
    'junk' (hard, 35 % inverted: beyond any code's reach)"""
    bits = np.unpackbits(np.asarray(frames, np.uint8), axis=1)[:, :framebits]
    hard = np.stack([O.encode(b) for b in bits]).astype(np.float64)
    if mode == "clean":
        return (hard * 255).astype(np.uint8)
    if mode in ("flip", "junk"):
        inv = rng.random(hard.shape) < (0.08 if mode == "flip" else 0.35)
        return (np.where(inv, 1 - hard, hard) * 255).astype(np.uint8)
    sigma = np.sqrt(1.0 / (2 * 0.25 * 10 ** 0.3))
    y = (2 * hard - 1) + sigma * rng.standard_normal(hard.shape)
    return np.clip(np.round(127.5 + 50 * y), 0, 255).astype(np.uint8)


def decodable_segments(rng, framebits):
    """a random profile of 1...4 segments in which every step keeps symbols 0 and 1 (the noise-free decode is unique)
    and a random choice of symbols 2 and 3"""
    T = framebits + TAIL
    nseg = int(rng.integers(1, 5))
    cuts = np.sort(rng.choice(np.arange(1, T), nseg - 1, replace=False)) if nseg > 1 else np.array([], np.int64)
    steps = np.diff(np.concatenate(([0], cuts, [T])))
    segs = []
    for s in steps:
        nibs = 3 | (rng.integers(0, 4, 8) << 2)
        segs.append((int(s), int(sum(int(v) << (4 * i) for i, v in enumerate(nibs)))))
    return segs


def fic_profile(framebits):
    return fic_segments() if framebits == 768 else [(framebits, KEEP_24), (TAIL, KEEP_TAIL_12)]


def fic_frames(rng, n, framebits):
    """n frames of random FIBs, each with a valid CRC -> (payloads (n, fibs, 30), descrambled frames)"""
    nf = framebits // 256
    pay = rng.integers(0, 256, (n, nf, 30), dtype=np.uint8)
    frames = np.stack([np.concatenate([make_fib(p) for p in fr]) for fr in pay])
    return pay, frames


def dev(a, offset=0):
    """host bytes -> a device view starting `offset` bytes into a fresh allocation"""
    a = np.ascontiguousarray(a, np.uint8).reshape(-1)
    buf = torch.empty(offset + a.size, dtype=torch.uint8, device="cuda")
    buf[offset:] = torch.from_numpy(a).cuda()
    return buf[offset:]


# ---- energy dispersal -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("framebits", [2, 8, 256, 768, 770, 1000, 2304, 9216])
def test_dispersal_uniform(V, torch_cuda, framebits):
    """odd base pointer, guard bytes on both sides; output = input XOR PRBS on the valid bits, padding bits and guards
    unchanged, twice = identity"""
    torch = torch_cuda
    rng = np.random.default_rng(framebits)
    nb = (framebits + 7) // 8
    for n in (1, 3, 4097):
        host = rng.integers(0, 256, GUARD + n * nb + GUARD, dtype=np.uint8)
        buf = dev(host, offset=3)
        frames = buf[GUARD:GUARD + n * nb]
        V.energy_dispersal_dev(frames, framebits, n)
        torch.cuda.synchronize()
        want = host.copy()
        want[GUARD:GUARD + n * nb] = scramble(host[GUARD:GUARD + n * nb].reshape(n, nb), framebits).reshape(-1)
        assert np.array_equal(buf.cpu().numpy(), want), (framebits, n)
        V.energy_dispersal_dev(frames, framebits, n)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), host), (framebits, n)


def test_dispersal_varlen(V, torch_cuda):
    """a mixed table: valid frames of many lengths at arbitrary offsets, 770-bit frames packed back to back (97 bytes
    apart: neighbours share dwords), and descriptors with odd or oversize framebits or output outside the buffer.
    Valid frames are descrambled; skipped frames and the gaps stay byte-identical."""
    torch = torch_cuda
    rng = np.random.default_rng(5)
    descs, pos, valid = [], 1, []
    for i in range(600):
        fb = int(rng.choice([2, 16, 256, 768, 770, 1000, 4608, 9216]))
        if i % 7 == 0:  # a run of back-to-back 770-bit frames
            for _ in range(5):
                descs.append((pos, 770))
                valid.append(True)
                pos += 97
        pos += int(rng.integers(0, 6))  # a gap
        descs.append((pos, fb))
        valid.append(True)
        pos += (fb + 7) // 8
    out_bytes = pos + 3
    host = rng.integers(0, 256, out_bytes + 40, dtype=np.uint8)  # 40 bytes past out_bytes: never touched
    bad = [(5, 767), (9, 9218), (11, 0xFFFFFFFE), (out_bytes - 96, 770), (out_bytes + 1, 2), (1 << 62, 768),
           ((1 << 64) - 8, 256), (out_bytes - 1, 16)]
    for d in bad:
        k = int(rng.integers(0, len(descs)))
        descs.insert(k, d)
        valid.insert(k, False)
    table = np.zeros(len(descs), V.DESC_DTYPE)
    table["out_offset"] = [d[0] for d in descs]
    table["framebits"] = [d[1] for d in descs]
    table["sym_offset"] = rng.integers(0, 1 << 62, len(descs), dtype=np.uint64)  # ignored
    table["reserved"] = 0xFFFFFFFF                                                 # ignored
    want = host.copy()
    for (oo, fb), ok in zip(descs, valid):
        if ok:
            nb = (fb + 7) // 8
            want[oo:oo + nb] = scramble(want[oo:oo + nb][None], fb)[0]
    # the last valid descriptor ends exactly at out_bytes: give it those bytes
    assert max(d[0] + (d[1] + 7) // 8 for d, ok in zip(descs, valid) if ok) <= out_bytes
    buf = dev(host, offset=1)
    d_desc = dev(table.view(np.uint8))
    V.energy_dispersal_varlen_dev(buf, d_desc, len(descs), out_bytes=out_bytes)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), want)
    assert np.array_equal(d_desc.cpu().numpy(), table.view(np.uint8))
    # a frame ending exactly at out_bytes is valid
    t1 = np.zeros(1, V.DESC_DTYPE)
    t1["out_offset"], t1["framebits"] = out_bytes - 97, 770
    before = buf.cpu().numpy()
    V.energy_dispersal_varlen_dev(buf, dev(t1.view(np.uint8)), 1, out_bytes=out_bytes)
    torch.cuda.synchronize()
    exp = before.copy()
    exp[out_bytes - 97:out_bytes] = scramble(before[out_bytes - 97:out_bytes][None], 770)[0]
    assert np.array_equal(buf.cpu().numpy(), exp)


# ---- FIB CRC --------------------------------------------------------------------------------------------------------

def test_fib_crc(V, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(6)
    good = np.stack([make_fib(rng.integers(0, 256, 30, dtype=np.uint8)) for _ in range(300)])
    flipped = np.repeat(good[:64], 4, axis=0)
    pos = rng.integers(0, 256, flipped.shape[0])
    flipped[np.arange(flipped.shape[0]), pos // 8] ^= (0x80 >> (pos % 8)).astype(np.uint8)
    rand = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    fibs = np.concatenate([good, flipped, rand])
    fibs = fibs[rng.permutation(fibs.shape[0])]
    want = fib_ok_model(fibs)
    assert want.sum() >= 300
    for offset in (0, 1, 3):
        d_f = dev(fibs, offset)
        d_ok = torch.full((fibs.shape[0] + 8,), 0xEE, dtype=torch.uint8, device="cuda")
        V.fib_crc_dev(d_f, fibs.shape[0], d_ok[1:])
        torch.cuda.synchronize()
        ok = d_ok.cpu().numpy()
        assert np.array_equal(ok[1:1 + fibs.shape[0]], want), offset
        assert ok[0] == 0xEE and (ok[1 + fibs.shape[0]:] == 0xEE).all()
        assert np.array_equal(d_f.cpu().numpy(), fibs.reshape(-1))


# ---- FIC chain ------------------------------------------------------------------------------------------------------

def run_fic(V, torch, d_in, n, framebits, profile, ge, offset=0):
    nb = framebits // 8
    d_f = torch.full((offset + n * nb + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((offset + n * (framebits // 256) + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    old = V.set_renorm_ge(ge)
    try:
        V.decode_fic_dev(d_in, d_f[offset:], d_ok[offset:], framebits, n, profile)
        torch.cuda.synchronize()
    finally:
        V.set_renorm_ge(old)
    f, ok = d_f.cpu().numpy(), d_ok.cpu().numpy()
    assert (f[:offset] == 0xEE).all() and (f[offset + n * nb:] == 0xEE).all()
    assert (ok[:offset] == 0xEE).all() and (ok[offset + n * (framebits // 256):] == 0xEE).all()
    return f[offset:offset + n * nb].reshape(n, nb), ok[offset:offset + n * (framebits // 256)]


@pytest.mark.parametrize("framebits", [768, 1024, 9216])
@pytest.mark.parametrize("ge", [False, True])
def test_fic_chain(V, O, torch_cuda, framebits, ge):
    """scrambled FIBs through the mother code, noise-free, at 3 dB and hard-flipped; punctured and unpunctured input;
    d_fibs = the oracle's decode XOR PRBS, d_fib_ok = the model's CRC on it; noise-free: the payloads come back"""
    torch = torch_cuda
    rng = np.random.default_rng(framebits + ge)
    n = 24 if framebits == 9216 else 60
    segs = fic_profile(framebits)
    for mode in ("clean", "3dB", "flip"):
        pay, frames = fic_frames(rng, n, framebits)
        sym = channel(O, scramble(frames, framebits), framebits, rng, mode)
        for profile in (segs, None):
            if profile is None:
                d_in, full = dev(sym), sym
            else:
                punct = puncture(sym, segs, framebits)
                d_in, full = dev(punct, offset=1), depuncture(punct, segs, framebits, 128)
            want = scramble(O.decode_batch(framebits, full, nthreads=8, ge=ge), framebits)
            want_ok = fib_ok_model(want.reshape(-1, 32))
            got, ok = run_fic(V, torch, d_in, n, framebits, profile, ge, offset=1)
            assert np.array_equal(got, want), (mode, profile is None)
            assert np.array_equal(ok, want_ok), (mode, profile is None)
            if mode == "clean":
                assert ok.all()
                assert np.array_equal(got.reshape(n, -1, 32)[:, :, :30], pay)
            if mode == "flip" and profile is not None:
                assert 0 < ok.sum() < ok.size  # some FIBs survive, some do not


def test_fic_chain_full_size(V, O, torch_cuda):
    """65536 FIC frames, 256 distinct ones tiled, punctured: every tile equals the oracle's decode XOR PRBS, every flag
    the model's"""
    torch = torch_cuda
    rng = np.random.default_rng(65536)
    framebits, base_n, reps = 768, 256, 256
    segs = fic_segments()
    _, frames = fic_frames(rng, base_n, framebits)
    modes = np.array(["clean", "3dB", "flip"])[np.arange(base_n) % 3]
    sym = np.concatenate([channel(O, scramble(frames[modes == m], framebits), framebits, rng, m)
                          for m in ("clean", "3dB", "flip")])
    punct = puncture(sym, segs, framebits)
    want = scramble(O.decode_batch(framebits, depuncture(punct, segs, framebits, 128), nthreads=8), framebits)
    want_ok = fib_ok_model(want.reshape(-1, 32)).reshape(base_n, 3)
    assert 0 < want_ok.sum() < want_ok.size
    n = base_n * reps
    d_in = torch.from_numpy(punct).cuda().repeat(reps, 1).contiguous()
    d_f = torch.zeros((n, 96), dtype=torch.uint8, device="cuda")
    d_ok = torch.full((n, 3), 0xEE, dtype=torch.uint8, device="cuda")
    V.decode_fic_dev(d_in, d_f, d_ok, framebits, n, segs)
    torch.cuda.synchronize()
    assert bool((d_f.view(reps, base_n, 96) == torch.from_numpy(want).cuda().unsqueeze(0)).all())
    assert bool((d_ok.view(reps, base_n, 3) == torch.from_numpy(want_ok).cuda().unsqueeze(0)).all())


# ---- DAB+ chain -----------------------------------------------------------------------------------------------------

def dabplus_superframes(rng, nsf, rsdims):
    """nsf superframes from their definition: 110*rsdims bytes whose bytes 0..10 carry a valid fire code, RS(120,110)
    column-wise -> (payloads (nsf, 110*rsdims), descrambled superframes (nsf, 120*rsdims))"""
    pay = np.stack([with_fire_code(rng.integers(0, 256, 110 * rsdims, dtype=np.uint8)) for _ in range(nsf)])
    cw = rs_encode_columns(pay.reshape(nsf, 110, rsdims).transpose(1, 0, 2).reshape(110, nsf * rsdims))
    sf = cw.reshape(120, nsf, rsdims).transpose(1, 0, 2).reshape(nsf, 120 * rsdims)
    return pay, np.ascontiguousarray(sf)


def dabplus_symbols(O, rng, sf, rsdims, modes):
    """superframes -> 5 scrambled frames each -> symbols per superframe mode"""
    fb = 192 * rsdims
    frames = scramble(sf.reshape(-1, 24 * rsdims), fb).reshape(sf.shape[0], 5, -1)
    return np.concatenate([channel(O, frames[i], fb, rng, m) for i, m in enumerate(modes)])


def run_dabplus(V, torch, d_in, profile, nsf, rsdims, ge=False, fire=True):
    d_work = torch.full((nsf, 120 * rsdims), 0xEE, dtype=torch.uint8, device="cuda")
    d_out = torch.full((nsf, 110 * rsdims), 0xA5, dtype=torch.uint8, device="cuda")
    d_ret = torch.full((nsf,), 0x7777, dtype=torch.int32, device="cuda")
    d_fire = torch.full((nsf + 1,), 0xEE, dtype=torch.uint8, device="cuda") if fire else None
    old = V.set_renorm_ge(ge)
    try:
        V.dabplus_punctured_superframes_dev(d_in, profile, d_work, d_out, d_ret, rsdims, nsf,
                                            d_fire_ok=None if d_fire is None else d_fire[:nsf])
        torch.cuda.synchronize()
    finally:
        V.set_renorm_ge(old)
    fire_ok = None
    if fire:
        f = d_fire.cpu().numpy()
        assert f[nsf] == 0xEE
        fire_ok = f[:nsf]
    return d_work.cpu().numpy(), d_out.cpu().numpy(), d_ret.cpu().numpy(), fire_ok


@pytest.mark.parametrize("rsdims", [1, 4, 8, 16, 48])
def test_dabplus_chain(V, O, torch_cuda, rsdims):
    """d_work = the oracle's decode XOR PRBS, d_rs_out / d_ret = the oracle's RS check of it (untouched columns keep
    their sentinel), d_fire_ok = the model; noise-free superframes give fire_ok 1 and their payload; a window shifted
    by one frame gives fire_ok 0; the fused call equals decode_punctured_dev + energy_dispersal_dev + rs_batch_dev"""
    torch = torch_cuda
    rng = np.random.default_rng(100 + rsdims)
    fb = 192 * rsdims
    nsf = 6 if rsdims >= 16 else 10
    pay, sf = dabplus_superframes(rng, nsf + 1, rsdims)
    modes = (["clean", "3dB", "junk", "flip"] * nsf)[:nsf] + ["clean"]
    sym = dabplus_symbols(O, rng, sf, rsdims, modes)  # ((nsf+1)*5, 4*(fb+6))
    segs = decodable_segments(rng, fb)
    punct = puncture(sym, segs, fb)
    P = punct.shape[1]
    full = depuncture(punct, segs, fb, 128)
    d_punct = dev(punct, offset=1)
    for ge in (False, True):
        work_ref = scramble(O.decode_batch(fb, full[:5 * nsf], nthreads=8, ge=ge), fb).reshape(nsf, -1)
        ret_ref, out_ref = O.rs_check_batch(work_ref, rsdims, out_init=np.full((nsf, 110 * rsdims), 0xA5, np.uint8))
        fire_ref = fire_ok_model(work_ref)
        work, out, ret, fire_ok = run_dabplus(V, torch, d_punct[:5 * nsf * P], segs, nsf, rsdims, ge=ge)
        assert np.array_equal(work, work_ref), ge
        assert np.array_equal(ret, ret_ref), ge
        assert np.array_equal(out, out_ref), ge
        assert np.array_equal(fire_ok, fire_ref), ge
        clean = np.array([m == "clean" for m in modes[:nsf]])
        assert fire_ok[clean].all() and np.array_equal(out[clean], pay[:nsf][clean]) and (ret[clean] == 0).all()
        assert (ret[np.array([m == "junk" for m in modes[:nsf]])] == -1).all()  # beyond RS capacity
    # unpunctured input, and no fire flags wanted
    work, out, ret, _ = run_dabplus(V, torch, dev(sym[:5 * nsf]), None, nsf, rsdims, fire=False)
    work_ref = scramble(O.decode_batch(fb, sym[:5 * nsf], nthreads=8), fb).reshape(nsf, -1)
    assert np.array_equal(work, work_ref)
    # a window one frame late: superframe starts are frames 1, 6, 11, ...
    _, _, _, fire_ok = run_dabplus(V, torch, d_punct[P:P + 5 * nsf * P], segs, nsf, rsdims)
    assert not fire_ok.any()
    # the fused call = the three separate calls, byte for byte
    work, out, ret, _ = run_dabplus(V, torch, d_punct[:5 * nsf * P], segs, nsf, rsdims)
    d_work = torch.full((nsf, 120 * rsdims), 0xEE, dtype=torch.uint8, device="cuda")
    d_out = torch.full((nsf, 110 * rsdims), 0xA5, dtype=torch.uint8, device="cuda")
    d_ret = torch.full((nsf,), 0x7777, dtype=torch.int32, device="cuda")
    V.decode_punctured_dev(d_punct[:5 * nsf * P], d_work, fb, 5 * nsf, segs)
    V.energy_dispersal_dev(d_work, fb, 5 * nsf)
    V.rs_batch_dev(d_work, d_out, d_ret, rsdims, nsf)
    torch.cuda.synchronize()
    assert np.array_equal(d_work.cpu().numpy(), work)
    assert np.array_equal(d_out.cpu().numpy(), out) and np.array_equal(d_ret.cpu().numpy(), ret)


# ---- arguments, streams ---------------------------------------------------------------------------------------------

def test_argument_errors(V, torch_cuda):
    torch = torch_cuda
    L = V.lib()
    d = torch.full((1 << 16,), 0x33, dtype=torch.uint8, device="cuda")
    d_ret = torch.full((4,), 0x33, dtype=torch.int32, device="cuda")
    segs = fic_segments()
    for fb in (0, 128, 770, 9472, 1 << 31):
        with pytest.raises(V.ViterbiError):
            V.decode_fic_dev(d, d, d, fb, 1, None)
    for rsdims in (0, 49, 1 << 20):
        with pytest.raises(V.ViterbiError):
            V.dabplus_punctured_superframes_dev(d, None, d, d, d_ret, rsdims, 1)
    with pytest.raises(V.ViterbiError):
        V.decode_fic_dev(d, d, d, 768, 1, [(773, 0xFFFFFFFF)])  # profile not covering 768 + 6 steps
    with pytest.raises(V.ViterbiError):
        V.dabplus_punctured_superframes_dev(d, [(100, 0xFFFFFFFF)], d, d, d_ret, 4, 1)
    for fb in (3, 9218):
        with pytest.raises(V.ViterbiError):
            V.energy_dispersal_dev(d, fb, 1)
    p = V.punct_profile(segs)
    import ctypes as C
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = C.c_void_p(d.data_ptr())
    assert L.vit_decode_fic_dev(None, ptr, ptr, 768, 1, None, 128, s) == 1
    assert L.vit_decode_fic_dev(None, ptr, ptr, 768, 1, C.byref(p), 128, s) == 1
    assert L.vit_decode_fic_dev(ptr, None, ptr, 768, 1, None, 128, s) == 1
    assert L.vit_decode_fic_dev(ptr, ptr, None, 768, 1, None, 128, s) == 1
    assert L.vit_dabplus_punctured_superframes_dev(None, None, 128, ptr, ptr, ptr, None, 4, 1, s) == 1
    assert L.vit_dabplus_punctured_superframes_dev(ptr, None, 128, None, ptr, ptr, None, 4, 1, s) == 1
    assert L.vit_dabplus_punctured_superframes_dev(ptr, None, 128, ptr, None, ptr, None, 4, 1, s) == 1
    assert L.vit_dabplus_punctured_superframes_dev(ptr, None, 128, ptr, ptr, None, None, 4, 1, s) == 1
    assert L.vit_energy_dispersal_dev(None, 768, 1, s) == 1
    assert L.vit_energy_dispersal_varlen_dev(ptr, 100, None, 1, s) == 1
    assert L.vit_fib_crc_dev(ptr, 1, None, s) == 1
    assert L.vit_fib_crc_dev(ptr, -1, ptr, s) == 1
    assert "bad arguments" in V.last_error()
    # empty batches: OK, nothing written
    V.decode_fic_dev(d, d, d, 768, 0, segs)
    V.dabplus_punctured_superframes_dev(d, segs, d, d, d_ret, 24, 0, d_fire_ok=d)
    V.energy_dispersal_dev(d, 768, 0)
    V.energy_dispersal_dev(d, 0, 5)
    V.energy_dispersal_varlen_dev(d, d, 0)
    V.fib_crc_dev(d, 0, d)
    torch.cuda.synchronize()
    assert bool((d == 0x33).all()) and bool((d_ret == 0x33).all())


def test_two_threads_interleave_both_chains(V, O, torch_cuda):
    """two threads, each on its own streams, alternating FIC and DAB+ chains of different sizes (punctured and not):
    every output correct - the scratch buffer and its event ordering hold"""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    fic = []
    for n in (2100, 37):
        _, frames = fic_frames(rng, 64, 768)
        sym = channel(O, scramble(frames, 768), 768, rng, "3dB")
        punct = puncture(sym, fic_segments(), 768)
        want = scramble(O.decode_batch(768, depuncture(punct, fic_segments(), 768, 128), nthreads=8), 768)
        reps = (n + 63) // 64
        d_in = torch.from_numpy(np.tile(punct, (reps, 1))[:n]).cuda()
        fic.append((n, d_in, np.tile(want, (reps, 1))[:n], np.tile(fib_ok_model(want.reshape(-1, 32)).reshape(64, 3),
                                                                    (reps, 1))[:n]))
    dab = []
    for rsdims, nsf, punctured in ((24, 8, True), (4, 20, False)):
        fb = 192 * rsdims
        _, sf = dabplus_superframes(rng, nsf, rsdims)
        sym = dabplus_symbols(O, rng, sf, rsdims, ["3dB"] * nsf)
        segs = decodable_segments(rng, fb) if punctured else None
        inp = puncture(sym, segs, fb) if punctured else sym
        full = depuncture(inp, segs, fb, 128) if punctured else sym
        work = scramble(O.decode_batch(fb, full, nthreads=8), fb).reshape(nsf, -1)
        ret, out = O.rs_check_batch(work, rsdims, out_init=np.zeros((nsf, 110 * rsdims), np.uint8))
        dab.append((rsdims, nsf, segs, torch.from_numpy(inp).cuda(), work, out, ret, fire_ok_model(work)))
    errs = []

    def work(tid):
        try:
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            outs = []
            for rep in range(6):
                st = streams[rep & 1]
                with torch.cuda.stream(st):
                    if (rep + tid) % 2 == 0:
                        n, d_in, want, want_ok = fic[(rep // 2) % 2]
                        d_f = torch.zeros((n, 96), dtype=torch.uint8, device="cuda")
                        d_ok = torch.zeros((n, 3), dtype=torch.uint8, device="cuda")
                        V.decode_fic_dev(d_in, d_f, d_ok, 768, n, fic_segments(), stream=st.cuda_stream)
                        outs.append(((d_f, want), (d_ok, want_ok)))
                    else:
                        rsdims, nsf, segs, d_in, w_work, w_out, w_ret, w_fire = dab[(rep // 2) % 2]
                        d_work = torch.zeros((nsf, 120 * rsdims), dtype=torch.uint8, device="cuda")
                        d_out = torch.zeros((nsf, 110 * rsdims), dtype=torch.uint8, device="cuda")
                        d_ret = torch.zeros(nsf, dtype=torch.int32, device="cuda")
                        d_fire = torch.zeros(nsf, dtype=torch.uint8, device="cuda")
                        V.dabplus_punctured_superframes_dev(d_in, segs, d_work, d_out, d_ret, rsdims, nsf,
                                                            d_fire_ok=d_fire, stream=st.cuda_stream)
                        outs.append(((d_work, w_work), (d_out, w_out), (d_ret, w_ret), (d_fire, w_fire)))
            torch.cuda.synchronize()
            for k, pairs in enumerate(outs):
                for j, (d, w) in enumerate(pairs):
                    if not np.array_equal(d.cpu().numpy(), w):
                        errs.append((tid, k, j))
        except Exception as e:  # noqa: BLE001
            errs.append((tid, repr(e)))

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
