"""GPU: DAB+ access units (vit_dabplus_aus_dev) and the per-frame fire code (vit_fire_code_dev) against the model and
the builder of tests/test_au_host.py: whole vit_au_table arrays byte for byte, sentinel records behind the batch and
the superframes themselves unchanged."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (torch's runtime first, as when the whole suite is collected)

from test_au_host import (AU_BAD_HEADER, AU_DTYPE, AU_OK, AU_RS_FAILED, HEADER_LEN, PARAM, au_table_model, make_superframe,
                          random_starts, same)
from test_dab_host import scramble
from test_gpu_dab import channel, dabplus_symbols, decodable_segments, dev
from test_punct_host import depuncture, puncture

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import rs_encode_columns  # noqa: E402

pytestmark = pytest.mark.gpu

REC = AU_DTYPE.itemsize  # 20


# ---- running ----------------------------------------------------------------------------------------------------------

def run_aus(V, torch, sfs, rsdims, offset=0, stride=None, ret=None):
    """superframes (n, 110*rsdims) laid out `stride` apart from `offset` bytes into an allocation -> the n records;
    checks the sentinel records around the batch and that the buffer is unchanged"""
    sfs = np.asarray(sfs, np.uint8)
    n, L = sfs.shape
    assert L == 110 * rsdims
    stride = L if stride is None else stride
    host = np.full(n * stride + 16, 0xC3, np.uint8)
    host[:n * stride].reshape(n, stride)[:, :L] = sfs
    d_sf = dev(host, offset)
    d_au = torch.full(((n + 2) * REC,), 0xEE, dtype=torch.uint8, device="cuda")
    d_ret = None if ret is None else torch.from_numpy(np.asarray(ret, np.int32)).cuda()
    V.dabplus_aus_dev(d_sf, rsdims, n, d_au[REC:], d_ret=d_ret, sf_stride=stride)
    torch.cuda.synchronize()
    au = d_au.cpu().numpy()
    assert (au[:REC] == 0xEE).all() and (au[(n + 1) * REC:] == 0xEE).all()
    assert np.array_equal(d_sf.cpu().numpy(), host)
    return au[REC:(n + 1) * REC].view(AU_DTYPE)


def starts_of(n, lengths):
    st = np.cumsum([HEADER_LEN[n]] + list(lengths))
    return [int(x) for x in st[1:-1]]


def with_flips(sf, n, full):
    """the superframe and, for each AU, copies with one bit flipped in its first payload byte, its last payload byte
    and each of its CRC bytes -> (copies, the crc_ok mask each must give)"""
    out, masks = [sf], [(1 << n) - 1]
    for k in range(n):
        for pos, bit in ((full[k], 0x80), (full[k + 1] - 3, 0x01), (full[k + 1] - 2, 0x10), (full[k + 1] - 1, 0x04)):
            c = sf.copy()
            c[pos] ^= bit
            out.append(c)
            masks.append(((1 << n) - 1) ^ (1 << k))
    return out, masks


# ---- directed, small --------------------------------------------------------------------------------------------------

SPECIAL = [3, 4, 5] + list(range(60, 71)) + list(range(125, 132))  # +2 CRC bytes: where a lane's chunk grows by a byte


@pytest.mark.parametrize("rsdims", [1, 2, 3])
def test_directed_lengths_and_flips(V, torch_cuda, rsdims):
    """all four num_aus; the first or the last AU of each special length, the AUs between of 3, 4 and 5 bytes; bases 0,
    1, 3 and strides L, L + 1, L + 10"""
    rng = np.random.default_rng(40 + rsdims)
    L = 110 * rsdims
    sfs, masks, seen = [], [], set()
    for n in (2, 3, 4, 6):
        short = [3 + (j % 3) for j in range(n - 2)]
        for ell in SPECIAL:
            rest = L - HEADER_LEN[n] - ell - sum(short)
            if rest < 3 or HEADER_LEN[n] + rest + sum(short) > 4095:
                continue
            for lengths in ([ell] + short + [rest], [rest] + short + [ell]):
                st = starts_of(n, lengths)
                sf = make_superframe(rng, rsdims, PARAM[n] | int(rng.integers(0, 32)), st)
                c, m = with_flips(sf, n, [HEADER_LEN[n]] + st + [L])
                sfs += c
                masks += m
                seen.update(lengths)
    assert rsdims == 1 or set(SPECIAL) <= seen
    assert {3, 4, 5} | set(range(60, 71)) <= seen
    sfs = np.stack(sfs)
    want = au_table_model(sfs, rsdims)
    assert (want["status"] == AU_OK).all() and want["crc_ok"].tolist() == masks
    for offset in (0, 1, 3):
        for stride in (L, L + 1, L + 10):
            got = run_aus(V, torch_cuda, sfs, rsdims, offset, stride)
            assert same(got, want), (offset, stride, np.flatnonzero(got != want)[:8])


def test_every_single_bit_flip(V, torch_cuda):
    """one 110-byte superframe of 6 AUs: each of the 792 single-bit flips of bytes 11..109 clears exactly one flag"""
    rng = np.random.default_rng(50)
    st = [20, 23, 45, 70, 90]
    sf = make_superframe(rng, 1, 0x40, st)
    flips = np.repeat(sf[None], 792, axis=0)
    pos = np.arange(792)
    flips[pos, 11 + pos // 8] ^= (0x80 >> (pos % 8)).astype(np.uint8)
    sfs = np.concatenate([sf[None], flips])
    want = au_table_model(sfs, 1)
    bounds = np.array([11] + st + [110])
    hit = np.searchsorted(bounds, 11 + pos // 8, side="right") - 1
    assert want["crc_ok"].tolist() == [63] + [63 ^ (1 << int(k)) for k in hit]
    assert same(run_aus(V, torch_cuda, sfs, 1, offset=1), want)


@pytest.mark.parametrize("rsdims,offset,extra", [(48, 0, 0), (37, 1, 1)])
def test_length_sweep(V, torch_cuda, rsdims, offset, extra):
    """num_aus 2: AU 0 of every length 3 ... 300 and the longest ones the 12-bit start allows, AU 1 the rest (up to 5272
    bytes at RSDims 48, the longest possible AU); RSDims 37 from an odd base at an odd stride"""
    rng = np.random.default_rng(60 + rsdims)
    L = 110 * rsdims
    top = min(4095, L - 3) - 5  # AU 0's greatest length
    lengths = list(range(3, 301)) + list(range(top - 10, top + 1))
    assert rsdims != 48 or lengths[-11:] == list(range(4080, 4091))
    sfs = np.stack([make_superframe(rng, rsdims, 0x20, [5 + ell]) for ell in lengths])
    sfs[1::2, L - 7] ^= 0x08  # every other one: AU 1 damaged near its end
    sfs[2::3, 6] ^= 0x40      # and AU 0 in every third
    want = au_table_model(sfs, rsdims)
    assert (want["status"] == AU_OK).all() and set(want["crc_ok"].tolist()) == {0, 1, 2, 3}
    assert int((want["au_start"][:, 2] - want["au_start"][:, 1]).max()) == L - 8
    assert same(run_aus(V, torch_cuda, sfs, rsdims, offset, L + extra), want)


# ---- random -----------------------------------------------------------------------------------------------------------

def random_batch(rng, rsdims, count):
    """half valid with random cuts, a quarter valid with one damaged AU, a quarter with random bytes 2..10"""
    L = 110 * rsdims
    sfs = []
    for i in range(count):
        n = (2, 3, 4, 6)[int(rng.integers(0, 4))]
        sf = make_superframe(rng, rsdims, PARAM[n] | int(rng.integers(0, 32)), random_starts(rng, rsdims, n))
        if i % 4 == 2:
            sf[int(rng.integers(HEADER_LEN[n], L))] ^= 1 << int(rng.integers(0, 8))
        elif i % 4 == 3:
            sf[2:11] = rng.integers(0, 256, 9, dtype=np.uint8)
        sfs.append(sf)
    return np.stack(sfs)


@pytest.mark.parametrize("rsdims", [1, 4, 8, 24, 37, 48])
def test_random(V, torch_cuda, rsdims):
    rng = np.random.default_rng(70 + rsdims)
    sfs = random_batch(rng, rsdims, 256)
    want = au_table_model(sfs, rsdims)
    assert int((want["status"] == AU_OK).sum()) >= 32 and int((want["status"] == AU_BAD_HEADER).sum()) >= 32
    assert same(run_aus(V, torch_cuda, sfs, rsdims, offset=rsdims & 3), want)


def test_rs_gating(V, torch_cuda):
    rng = np.random.default_rng(80)
    sfs = random_batch(rng, 4, 40)
    ret = rng.integers(0, 6, 40).astype(np.int32)
    ret[[0, 3, 4, 17, 39]] = -1
    want = au_table_model(sfs, 4, ret)
    assert (want["status"][[0, 3, 4, 17, 39]] == AU_RS_FAILED).all()
    assert not want[[0, 3, 4, 17, 39]].view(np.uint8).reshape(5, REC)[:, 1:].any()
    assert same(run_aus(V, torch_cuda, sfs, 4, ret=ret), want)
    free = au_table_model(sfs, 4)
    assert same(run_aus(V, torch_cuda, sfs, 4, ret=np.abs(ret)), free)
    assert same(run_aus(V, torch_cuda, sfs, 4, ret=None), free)


# ---- after the chain --------------------------------------------------------------------------------------------------

def test_after_the_chain(V, O, torch_cuda):
    """superframes of built AUs through RS encoding, scrambling, the mother code, a channel and puncturing; the chain,
    then the AU pass on d_rs_out with d_ret, and on d_work at stride 120*RSDims (the salvage form)"""
    torch = torch_cuda
    rng = np.random.default_rng(90)
    rsdims, nsf = 4, 8
    fb, L = 192 * rsdims, 110 * rsdims
    heads = [(n, random_starts(rng, rsdims, n)) for n in (2, 3, 4, 6, 6, 4, 3, 2)]
    pay = np.stack([make_superframe(rng, rsdims, PARAM[n], st) for n, st in heads])
    cw = rs_encode_columns(pay.reshape(nsf, 110, rsdims).transpose(1, 0, 2).reshape(110, nsf * rsdims))
    sf = np.ascontiguousarray(cw.reshape(120, nsf, rsdims).transpose(1, 0, 2).reshape(nsf, 120 * rsdims))
    modes = ["clean", "3dB", "junk", "flip"] * 2
    sym = dabplus_symbols(O, rng, sf, rsdims, modes)
    segs = decodable_segments(rng, fb)
    punct = puncture(sym, segs, fb)
    work_ref = scramble(O.decode_batch(fb, depuncture(punct, segs, fb, 128), nthreads=8), fb).reshape(nsf, -1)
    ret_ref, out_ref = O.rs_check_batch(work_ref, rsdims, out_init=np.full((nsf, L), 0xA5, np.uint8))
    d_work = torch.full((nsf, 120 * rsdims), 0xEE, dtype=torch.uint8, device="cuda")
    d_out = torch.full((nsf, L), 0xA5, dtype=torch.uint8, device="cuda")
    d_ret = torch.full((nsf,), 0x7777, dtype=torch.int32, device="cuda")
    d_au = torch.full(((nsf + 1) * REC,), 0xEE, dtype=torch.uint8, device="cuda")
    d_salv = torch.full(((nsf + 1) * REC,), 0xEE, dtype=torch.uint8, device="cuda")
    V.dabplus_punctured_superframes_dev(dev(punct, offset=1), segs, d_work, d_out, d_ret, rsdims, nsf)
    V.dabplus_aus_dev(d_out, rsdims, nsf, d_au, d_ret=d_ret)
    V.dabplus_aus_dev(d_work, rsdims, nsf, d_salv, sf_stride=120 * rsdims)
    torch.cuda.synchronize()
    assert np.array_equal(d_ret.cpu().numpy(), ret_ref) and np.array_equal(d_out.cpu().numpy(), out_ref)
    assert np.array_equal(d_work.cpu().numpy(), work_ref)
    au, salv = d_au.cpu().numpy(), d_salv.cpu().numpy()
    assert (au[nsf * REC:] == 0xEE).all() and (salv[nsf * REC:] == 0xEE).all()
    au, salv = au[:nsf * REC].view(AU_DTYPE), salv[:nsf * REC].view(AU_DTYPE)
    assert same(au, au_table_model(out_ref, rsdims, ret_ref))
    assert same(salv, au_table_model(work_ref[:, :L], rsdims))
    for i, (n, st) in enumerate(heads):
        if modes[i] == "clean":
            assert au[i]["status"] == AU_OK and au[i]["crc_ok"] == (1 << n) - 1 and au[i]["fire_ok"] == 1
            assert au[i]["au_start"][:n + 1].tolist() == [HEADER_LEN[n]] + st + [L]
            assert np.array_equal(out_ref[i], pay[i]) and same(salv[i:i + 1], au[i:i + 1])
        if modes[i] == "junk":
            assert au[i]["status"] == AU_RS_FAILED and ret_ref[i] < 0


# ---- the fire code per frame ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rsdims", [2, 24])
def test_fire_code_per_frame(V, torch_cuda, rsdims):
    """17 descrambled frames whose superframes start at frame 2: flags 1 exactly at frames 2, 7 and 12"""
    torch = torch_cuda
    rng = np.random.default_rng(100 + rsdims)
    nb = 24 * rsdims
    frames = rng.integers(0, 256, (17, nb), dtype=np.uint8)
    for k in (2, 7, 12):
        frames[k:k + 5].reshape(-1)[:110 * rsdims] = make_superframe(rng, rsdims, 0x40, random_starts(rng, rsdims, 6))
    want = np.zeros(17, np.uint8)
    want[[2, 7, 12]] = 1
    for offset in (0, 1, 3):
        d_f = dev(frames, offset)
        d_ok = torch.full((17 + 8,), 0xEE, dtype=torch.uint8, device="cuda")
        V.fire_code_dev(d_f, nb, 17, d_ok[3:])
        torch.cuda.synchronize()
        ok = d_ok.cpu().numpy()
        assert ok[3:20].tolist() == want.tolist(), offset
        assert (ok[:3] == 0xEE).all() and (ok[20:] == 0xEE).all()
        assert np.array_equal(d_f.cpu().numpy(), frames.reshape(-1))


# ---- full size --------------------------------------------------------------------------------------------------------

def test_full_size(V, torch_cuda):
    """16384 superframes at RSDims 24, 64 distinct ones tiled; compared on the device"""
    torch = torch_cuda
    rng = np.random.default_rng(110)
    base, reps, rsdims = 64, 256, 24
    sfs = random_batch(rng, rsdims, base)
    ret = np.zeros(base, np.int32)
    ret[[5, 40]] = -1
    want = au_table_model(sfs, rsdims, ret)
    assert {AU_OK, AU_BAD_HEADER, AU_RS_FAILED} <= set(want["status"].tolist())
    d_sf = torch.from_numpy(sfs).cuda().repeat(reps, 1).contiguous()
    d_ret = torch.from_numpy(ret).cuda().repeat(reps).contiguous()
    d_au = torch.full((base * reps + 1, REC), 0xEE, dtype=torch.uint8, device="cuda")
    V.dabplus_aus_dev(d_sf, rsdims, base * reps, d_au, d_ret=d_ret)
    torch.cuda.synchronize()
    d_want = torch.from_numpy(want.view(np.uint8).reshape(base, REC)).cuda()
    assert bool((d_au[:-1].view(reps, base, REC) == d_want.unsqueeze(0)).all())
    assert bool((d_au[-1] == 0xEE).all())
    assert bool((d_sf.view(reps, base, -1) == torch.from_numpy(sfs).cuda().unsqueeze(0)).all())


# ---- arguments, streams -----------------------------------------------------------------------------------------------

def test_argument_errors(V, torch_cuda):
    torch = torch_cuda
    L = V.lib()
    d = torch.full((1 << 16,), 0x33, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr, odd = C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr() + 2)
    out = C.c_void_p(d.data_ptr() + 32768)
    assert L.vit_dabplus_aus_dev(None, 2640, 24, 1, None, out, s) == 1
    assert L.vit_dabplus_aus_dev(ptr, 2640, 24, 1, None, None, s) == 1
    assert L.vit_dabplus_aus_dev(ptr, 2640, 24, 1, None, odd, s) == 1       # d_au not 4-byte aligned
    assert L.vit_dabplus_aus_dev(ptr, 2640, 24, 1, None, C.c_void_p(d.data_ptr() + 32769), s) == 1
    assert L.vit_dabplus_aus_dev(ptr, 2639, 24, 1, None, out, s) == 1       # stride shorter than a superframe
    assert L.vit_dabplus_aus_dev(ptr, 0, 1, 1, None, out, s) == 1
    assert L.vit_dabplus_aus_dev(ptr, 110 * 49, 49, 1, None, out, s) == 1   # RSDims 1 ... 48
    assert L.vit_dabplus_aus_dev(ptr, 110, 0, 1, None, out, s) == 1
    assert L.vit_dabplus_aus_dev(ptr, 2640, 24, -1, None, out, s) == 1
    assert "vit_dabplus_aus_dev: bad arguments" in V.last_error()
    assert L.vit_fire_code_dev(None, 48, 1, out, s) == 1
    assert L.vit_fire_code_dev(ptr, 48, 1, None, s) == 1
    assert L.vit_fire_code_dev(ptr, 48, -1, out, s) == 1
    assert "vit_fire_code_dev: bad arguments" in V.last_error()
    with pytest.raises(V.ViterbiError):
        V.dabplus_aus_dev(d, 24, 1, d, sf_stride=100)
    # empty batches: OK, nothing written
    V.dabplus_aus_dev(d, 24, 0, d)
    V.fire_code_dev(d, 48, 0, d)
    assert L.vit_dabplus_aus_dev(None, 2640, 24, 0, None, None, s) == 0
    torch.cuda.synchronize()
    assert bool((d == 0x33).all())


def test_two_streams_in_issue_order(V, torch_cuda):
    """on each of two streams: fill the buffer, AU pass, refill the same buffer, AU pass - every table is that of the
    superframes its call was issued behind"""
    torch = torch_cuda
    rng = np.random.default_rng(120)
    rsdims, n = 24, 2048
    jobs = []
    for k in range(2):
        a, b = random_batch(rng, rsdims, 32), random_batch(rng, rsdims, 32)
        jobs.append((torch.cuda.Stream(), [torch.from_numpy(np.tile(x, (n // 32, 1))).cuda() for x in (a, b)],
                     [np.tile(au_table_model(x, rsdims), n // 32) for x in (a, b)],
                     torch.zeros((n, 110 * rsdims), dtype=torch.uint8, device="cuda"),
                     [torch.full((n * REC,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]))
    torch.cuda.synchronize()
    for rep in range(2):
        for st, src, _, d_buf, d_au in jobs:
            with torch.cuda.stream(st):
                d_buf.copy_(src[rep], non_blocking=True)
                V.dabplus_aus_dev(d_buf, rsdims, n, d_au[rep], stream=st.cuda_stream)
    torch.cuda.synchronize()
    for _, _, want, _, d_au in jobs:
        for rep in range(2):
            assert same(d_au[rep].cpu().numpy().view(AU_DTYPE), want[rep])
