"""CPU-only: "Integer sample formats" (include/viterbi_amd.h) - the one line in front of the front end's definition as a
numpy float32 model (convert_model), pinned against binary64 for every byte and every int16 value, the quantiser the GPU
tests draw their inputs from (a noise-free frame rounded to each format still demaps to the transmitted bits through the
existing models), the four exports and their failure without a device.  tests/test_gpu_iqfmt.py uses convert_model in
front of front_model, demap_model and sync_model as its exact reference."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_fft_host import front_model, time_domain, twiddles_model, useful_parts
from test_ofdm_host import demap_model, freq_bins_model, transmit

F32 = np.float32
IQ_F32, IQ_CU8, IQ_CS8, IQ_CS16 = 0, 1, 2, 3
INT_FORMATS = (IQ_CU8, IQ_CS8, IQ_CS16)
DTYPES = {IQ_CU8: np.uint8, IQ_CS8: np.int8, IQ_CS16: np.int16}
USUAL_SCALE = {IQ_CU8: 2.0 ** -8, IQ_CS8: 2.0 ** -7, IQ_CS16: 2.0 ** -15}  # full range is about +-1
SCALES = (1.0, 2.0 ** -8, 2.0 ** -15, float(F32(1.0 / 255.0)), float(F32(1.0 / 32768.0 * 1.5)))
NEW_EXPORTS = ("vit_ofdm_fft_iq_dev", "vit_ofdm_demod_iq_dev", "vit_ofdm_sync_iq_dev", "vit_iq_convert_dev")


# ---- the definition -------------------------------------------------------------------------------------------------

def convert_model(raw, fmt, scale):
    """raw: (..., 2) integers of the format's type, (I, Q) -> (...) complex64: one exact conversion and one float32
    multiplication per component"""
    raw = np.asarray(raw)
    assert raw.dtype == DTYPES[fmt] and raw.shape[-1] == 2
    i = raw.astype(np.int32)
    if fmt == IQ_CU8:
        i = 2 * i - 255
    v = i.astype(F32) * F32(scale)
    assert v.dtype == F32
    out = np.empty(raw.shape[:-1], np.complex64)
    out.real, out.imag = v[..., 0], v[..., 1]
    return out


def quantise(x, fmt, fill=0.9):
    """complex samples -> (raw (..., 2) of the format's type, scale): the largest component at `fill` of full range, every
    component rounded to the nearest code; scale brings full range back to about +-1"""
    x = np.asarray(x, np.complex128)
    v = np.stack([x.real, x.imag], axis=-1) * (fill / max(np.abs(x.real).max(), np.abs(x.imag).max()))
    if fmt == IQ_CU8:
        raw = np.clip(np.rint(v * 127.5 + 127.5), 0, 255)
    elif fmt == IQ_CS8:
        raw = np.clip(np.rint(v * 127.0), -128, 127)
    else:
        raw = np.clip(np.rint(v * 32767.0), -32768, 32767)
    return raw.astype(DTYPES[fmt]), USUAL_SCALE[fmt]


def all_codes(fmt):
    """every value of the format's type, as (I, Q) pairs: (n/2, 2)"""
    info = np.iinfo(DTYPES[fmt])
    return np.arange(info.min, info.max + 1).astype(DTYPES[fmt]).reshape(-1, 2)


# ---- the model against binary64 -------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", INT_FORMATS)
@pytest.mark.parametrize("scale", SCALES)
def test_convert_model_against_binary64(fmt, scale):
    """all 256 bytes and all 65536 int16 values: exact for a power of two, binary64 rounded once otherwise"""
    raw = all_codes(fmt)
    got = convert_model(raw, fmt, scale).view(F32).reshape(-1)
    i = raw.reshape(-1).astype(np.int64)
    if fmt == IQ_CU8:
        i = 2 * i - 255
    assert float(F32(scale)) == scale
    exact = i.astype(np.float64) * np.float64(scale)  # at most 17 bits times 24 bits: no rounding in binary64
    if np.log2(scale) == np.rint(np.log2(scale)):
        assert np.array_equal(got.astype(np.float64), exact)
    else:
        assert np.array_equal(got, exact.astype(F32))
    if fmt == IQ_CU8:
        assert (got != 0).all(), "no CU8 sample is 0"
        assert got.min() == F32(-255 * scale) and got.max() == F32(255 * scale)
    else:
        assert (got == 0).sum() == 1
    # inside the front end's domain at the ends of the scale's range too
    for s in (2.0 ** -32, 2.0 ** 16):
        m = np.abs(convert_model(raw, fmt, s).view(F32))
        assert ((m == 0) | ((m >= 2.0 ** -40) & (m <= 2.0 ** 40))).all()


# ---- the quantised inputs mean something ----------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", INT_FORMATS)
def test_quantised_frame_demaps_to_the_transmitted_bits(fmt):
    """a noise-free frame at nfft 256, 8 symbols, at 90 % of full range, rounded to the format: the model chain makes the
    decisions of the transmitted bits, 0 errors - a condition of the tests' inputs, not a tolerance"""
    shape, guard = (256, 192, 8, 3, 1), 63
    nfft, K, nsyms = shape[0], shape[1], shape[2]
    rng = np.random.default_rng(50 + fmt)
    bins = freq_bins_model(nfft)[1]
    bits = rng.integers(0, 2, (2, nsyms - 1, 2 * K))
    x = time_domain(transmit(bits, bins, shape, rng), guard)
    raw, scale = quantise(x, fmt)
    info = np.iinfo(DTYPES[fmt])
    assert raw.min() > info.min and raw.max() < info.max, "nothing clips at 90 %"
    xq = convert_model(raw, fmt, scale)
    assert 0.85 < max(np.abs(xq.real).max(), np.abs(xq.imag).max()) < 0.95
    tw, ss = twiddles_model(nfft), nfft + guard
    parts = np.stack([useful_parts(xq[t], guard // 2, shape, ss) for t in range(2)])
    out = demap_model(front_model(parts, tw), bins, shape, 254.0)
    assert np.array_equal(out > 128, bits.astype(bool))


# ---- the library without a GPU --------------------------------------------------------------------------------------

def test_iqfmt_exports(V):
    out = subprocess.check_output(["nm", "-D", "--defined-only", V.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW_EXPORTS:
        assert name in exported and name in V.EXPORTS
    assert (V.IQ_F32, V.IQ_CU8, V.IQ_CS8, V.IQ_CS16) == (IQ_F32, IQ_CU8, IQ_CS8, IQ_CS16)
    assert C.sizeof(V.IqFormat) == 8 and V.IqFormat.scale.offset == 4


def iq_calls(V, fmt, inp=None, buf=None):
    """the four calls with the given vit_iq_format (or None) and otherwise NULL buffers -> their return values and texts"""
    L = V.lib()
    inp = V.IqInput() if inp is None else inp
    inp.sym_stride, inp.frame_stride = 2552, 196608
    shape = V.OfdmShape(2048, 1536, 76, 3, 4)
    par = V.SyncParams(2048, 76, 75, 100, 16, 0.5, 0, 100)
    f = None if fmt is None else C.byref(fmt)
    out = []
    for rc in (lambda: L.vit_ofdm_fft_iq_dev(C.byref(inp), f, 2048, 76, 1, buf, 2048, 76 * 2048, None),
               lambda: L.vit_ofdm_demod_iq_dev(C.byref(inp), f, buf, C.byref(shape), 254.0, 1, buf, None, 0, None),
               lambda: L.vit_ofdm_sync_iq_dev(C.byref(inp), f, C.byref(par), buf, 1, buf, buf, None, None),
               lambda: L.vit_iq_convert_dev(buf, f, 16, buf, None)):
        out.append((rc(), V.last_error()))
    return out


def test_iqfmt_calls_fail_loudly(V):
    """without a device every new call returns VIT_ERR_NO_DEVICE and names gfx950, whatever its arguments; with one, a NULL
    fmt, format 4 and the scales 0, NaN, 2^-33 and 2^17 are VIT_ERR_ARG in front of every other rule - the buffers are
    NULL, so nothing is launched either way"""
    import torch
    want = 1 if torch.cuda.is_available() else 2  # VIT_ERR_ARG / VIT_ERR_NO_DEVICE
    bad = [None, V.IqFormat(4, 1.0), V.IqFormat(0xFFFFFFFF, 1.0)]
    for fmt in INT_FORMATS:
        bad += [V.IqFormat(fmt, s) for s in (0.0, float("nan"), 2.0 ** -33, 2.0 ** 17, -1.0, float("inf"))]
    for fmt in bad:
        for rc, text in iq_calls(V, fmt):
            assert rc == want
            assert ("fmt" in text or "format" in text or "scale" in text) if want == 1 else "gfx950" in text
    # a good format in front of NULL buffers: the existing rules
    for fmt in (V.IqFormat(V.IQ_CU8, 2.0 ** -8), V.IqFormat(V.IQ_CS16, 2.0 ** 16), V.IqFormat(V.IQ_F32, float("nan"))):
        for rc, text in iq_calls(V, fmt):
            assert rc == want
            assert "bad arguments" in text if want == 1 else "gfx950" in text
