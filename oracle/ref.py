"""Build recipe and ctypes front-end of oracle/_ref -- TEST INFRASTRUCTURE ONLY, like oracle.py.

oracle/_ref/ holds two shared objects made from the REFERENCE'S OWN deconvolve.cpp and rschecksf.cpp (compiled in
place from a reference checkout with -D_VIT_NO_ASM_, i.e. its C decoders) and this repository's harness
(oracle/ref/harness.cpp, stand-in headers under oracle/ref/shim/):

  libvitref.so       the reference as it is: renormalise when state 0's metric is `> 150`
  libvitref_t149.so  the same with RENORMALIZE_THRESHOLD 149: `> 149`, which for integers is the MASM decoders' `>= 150`

Neither is committed (oracle/_ref/ is ignored by git); what they computed is, as data, under tests/golden/
(tests/golden/make_reference_golden.py).  The checkout is looked for in $VIT_REFERENCE_DIR, then beside this
repository (../reference).  Without a checkout build() leaves existing libraries alone.
"""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
REF_DIR = os.path.join(_HERE, "_ref")
SO = {150: os.path.join(REF_DIR, "libvitref.so"), 149: os.path.join(REF_DIR, "libvitref_t149.so")}
_SRC = os.path.join(_HERE, "ref")
REFERENCE_TAG = "2024_10_08"
VARIANTS = ("sse2_lut32", "ssse3", "avx", "avx2", "avx5")
# SURVEY Appendix C.2.  -msse2 is the right baseline: every decoder carries its own target attribute.  -fno-exceptions
# keeps the C++ personality routine (libstdc++) out of the objects; nothing in the two files can throw.
CXXFLAGS = ["-fms-extensions", "-fdeclspec", "-std=c++17", "-O2", "-msse2", "-fPIC", "-fno-exceptions", "-D_VIT_NO_ASM_"]
# rschecksf.cpp only: its DECODE_RS is `__forceinline`, so no callable copy would be emitted for the one-codeword
# export; with the keyword defined away it is an ordinary function (same statements, same arithmetic)
RS_EXTRA = ["-D__forceinline="]
_REF_SOURCES = ("deconvolve.cpp", "rschecksf.cpp", "viterbi.h")
_THRESHOLD_LINE = "#define RENORMALIZE_THRESHOLD 150"


def reference_dir():
    """the reference checkout, or None"""
    for d in (os.environ.get("VIT_REFERENCE_DIR"), os.path.join(os.path.dirname(_ROOT), "reference")):
        if d and all(os.access(os.path.join(d, f), os.R_OK) for f in _REF_SOURCES):
            return d
    return None


def _tool(name):
    env = os.environ.get("VITREF_" + name.upper().replace("+", "X").replace("-", "_"))
    if env:
        return env
    for d in ("/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name)


def available():
    return all(os.path.exists(p) for p in SO.values())


def _stale(ref):
    if not available():
        return True
    t = min(os.path.getmtime(p) for p in SO.values())
    deps = [os.path.abspath(__file__), os.path.join(_SRC, "harness.cpp")]
    deps += [os.path.join(_SRC, "shim", f) for f in ("windows.h", "psapi.h", "intrin.h")]
    deps += [os.path.join(ref, f) for f in _REF_SOURCES]
    return any(os.path.getmtime(d) > t for d in deps)


def _lines_changed(orig_paths, new_paths):
    """number of lines that differ between the originals and the build-time copies"""
    n = 0
    for a, b in zip(orig_paths, new_paths):
        la, lb = open(a, "rb").read().split(b"\n"), open(b, "rb").read().split(b"\n")
        assert len(la) == len(lb), "the copy of %s has a different number of lines" % a
        n += sum(x != y for x, y in zip(la, lb))
    return n


def _build_one(ref, threshold, cxx, tmp):
    work = os.path.join(tmp, "t%d" % threshold)
    os.makedirs(work)
    inc = ["-I", os.path.join(_SRC, "shim")]
    if threshold == 150:
        decon = os.path.join(ref, "deconvolve.cpp")  # compiled in place: `#include "viterbi.h"` finds its neighbour
    else:
        # viterbi.h defines the macro unguarded, and the quoted include finds the file NEXT TO deconvolve.cpp first: so the
        # build compiles copies of the two (never committed, removed with the temporary directory), one line changed
        origs = [os.path.join(ref, f) for f in ("viterbi.h", "deconvolve.cpp")]
        copies = [os.path.join(work, f) for f in ("viterbi.h", "deconvolve.cpp")]
        text = open(origs[0], "rb").read()
        assert text.count(_THRESHOLD_LINE.encode()) == 1, "viterbi.h: expected exactly one `%s`" % _THRESHOLD_LINE
        with open(copies[0], "wb") as f:
            f.write(text.replace(_THRESHOLD_LINE.encode(), b"#define RENORMALIZE_THRESHOLD %d" % threshold))
        shutil.copyfile(origs[1], copies[1])
        assert _lines_changed(origs, copies) == 1, "the threshold build must differ from the reference in exactly one line"
        decon = copies[1]
    objs = []
    for name, src, extra in (("deconvolve", decon, []), ("rschecksf", os.path.join(ref, "rschecksf.cpp"), RS_EXTRA),
                             ("harness", os.path.join(_SRC, "harness.cpp"), ["-DREF_RENORM_THRESHOLD=%d" % threshold, "-Wall"])):
        obj = os.path.join(work, name + ".o")
        subprocess.check_call([cxx] + CXXFLAGS + extra + inc + ["-I", ref, "-c", src, "-o", obj])
        objs.append(obj)
    out = os.path.join(work, os.path.basename(SO[threshold]))
    # the three objects use no C++ run-time, and the library must load where it cannot be rebuilt: libc (with pthreads) only
    subprocess.check_call([cxx, "-shared", "-nostdlib++", "-Wl,--no-undefined", "-Wl,--as-needed", "-o", out] + objs + ["-lpthread"])
    readelf = _tool("llvm-readelf") or shutil.which("readelf")
    if readelf:
        needed = [l.split("[")[1].split("]")[0] for l in subprocess.check_output([readelf, "-d", out], text=True).splitlines()
                  if "NEEDED" in l]
        bad = [n for n in needed if not n.startswith(("libc.so", "libpthread.so", "ld-linux"))]
        assert not bad, "libvitref must depend on libc/libpthread only, found %s" % bad
    return out


def build(force=False):
    """-> True when oracle/_ref holds both libraries afterwards.  Needs the reference checkout to (re)build; without one
    an existing oracle/_ref is left as it is (a GPU machine: the libraries travel there, the checkout does not)."""
    ref = reference_dir()
    if ref is None:
        return available()
    if not force and not _stale(ref):
        return True
    cxx = _tool("clang++")
    if not cxx:
        raise RuntimeError("oracle/ref.py: no clang++ found (set VITREF_CLANGXX)")
    os.makedirs(REF_DIR, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="vitref_build_")
    try:
        built = {t: _build_one(ref, t, cxx, tmp) for t in (150, 149)}
        for t, p in built.items():
            os.replace(shutil.copyfile(p, SO[t] + ".tmp"), SO[t])
        with open(os.path.join(REF_DIR, "BUILD_INFO.txt"), "w") as f:
            ver = subprocess.check_output([cxx, "--version"], text=True).splitlines()[0]
            f.write("compiler: %s\nflags: %s\nreference tag: %s\n" % (ver, " ".join(CXXFLAGS), REFERENCE_TAG))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return True


def build_info():
    p = os.path.join(REF_DIR, "BUILD_INFO.txt")
    return dict(l.rstrip("\n").split(": ", 1) for l in open(p)) if os.path.exists(p) else {}


_libs = {}


def lib(threshold=150):
    if threshold not in _libs:
        if not os.path.exists(SO[threshold]):
            raise RuntimeError("%s not built: run oracle/ref.py build() next to a reference checkout" % SO[threshold])
        L = C.CDLL(SO[threshold])
        vp = C.c_void_p
        L.ref_decon.argtypes = [C.c_int, C.c_uint, vp, vp]
        L.ref_deconvolve.argtypes = [C.c_int, C.c_uint, vp, vp]
        for v in VARIANTS:
            getattr(L, "ref_decon_" + v).argtypes = [C.c_uint, vp, vp]
        L.ref_decode_batch_u8.argtypes = [C.c_int, C.c_uint, vp, vp, C.c_long, C.c_int]
        L.ref_rs_check_superframe.argtypes = [vp, C.c_int, C.c_uint, vp]
        L.ref_rs_check_batch.argtypes = [vp, C.c_uint, vp, vp, C.c_long]
        L.ref_rs_check_batch.restype = None
        L.ref_decode_rs.argtypes = [vp]
        L.ref_decode_rs_batch.argtypes = [vp, vp, C.c_long]
        L.ref_decode_rs_batch.restype = None
        L.ref_tables.argtypes = [vp, vp]
        L.ref_tables.restype = None
        L.ref_max_framebits.restype = C.c_uint
        assert L.ref_renorm_threshold() == threshold
        _libs[threshold] = L
    return _libs[threshold]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def variants(framebits=0):
    """names of the C decoder variants this CPU can run (and that can take a frame of that length: the 128-bit ones
    stop at 9214 bits, see ref_maxbits in harness.cpp)"""
    return [v for i, v in enumerate(VARIANTS) if lib().ref_variant_supported(i) and framebits <= lib().ref_max_framebits(i)]


def sym_len(framebits):
    return 4 * (framebits + 6)


def decode_batch(framebits, sym_u8, variant=None, ge=False, nthreads=4):
    """sym_u8: (nframes, 4*(framebits+6)) uint8 -> (nframes, (framebits+7)//8) uint8, like oracle.decode_batch.
    ge: the build with RENORMALIZE_THRESHOLD 149 (`>= 150`)"""
    sym_u8 = np.ascontiguousarray(sym_u8, np.uint8).reshape(-1, sym_len(framebits))
    n = sym_u8.shape[0]
    out = np.zeros((n, (framebits + 7) // 8), np.uint8)
    variant = variant or variants(framebits)[0]
    rc = lib(149 if ge else 150).ref_decode_batch_u8(VARIANTS.index(variant), framebits, _p(sym_u8), _p(out), n, nthreads)
    if rc != 0:
        raise RuntimeError("reference decode failed rc=%d (variant %s)" % (rc, variant))
    return out


def deconvolve_u32(framebits, sym_u32, variant=None, ge=False, dispatcher=False):
    """one frame in the reference ABI (u32 per symbol); dispatcher: through the DLL's `deconvolve` entry"""
    sym_u32 = np.ascontiguousarray(sym_u32, np.uint32)
    assert sym_u32.size >= sym_len(framebits)
    out = np.zeros((framebits + 7) // 8, np.uint8)
    L = lib(149 if ge else 150)
    variant = variant or variants(framebits)[0]
    fn = L.ref_deconvolve if dispatcher else L.ref_decon
    rc = fn(VARIANTS.index(variant), framebits, _p(sym_u32), _p(out))
    if rc != 0:
        raise RuntimeError("reference decode failed rc=%d (variant %s)" % (rc, variant))
    return out


def rs_check_superframe(p, rsdims, out=None):
    p = np.ascontiguousarray(p, np.uint8)
    assert p.size == 120 * rsdims
    if out is None:
        out = np.zeros(110 * rsdims, np.uint8)
    rc = lib().ref_rs_check_superframe(_p(p), 0, rsdims, _p(out))
    return rc, out


def rs_check_batch(p, rsdims, out_init=None):
    """p: (nsf, 120*rsdims) -> (ret[nsf] int32, out (nsf,110*rsdims)), like oracle.rs_check_batch"""
    p = np.ascontiguousarray(p, np.uint8).reshape(-1, 120 * rsdims)
    n = p.shape[0]
    out = (np.zeros((n, 110 * rsdims), np.uint8) if out_init is None
           else np.array(out_init, np.uint8).reshape(n, 110 * rsdims).copy())
    ret = np.zeros(n, np.int32)
    lib().ref_rs_check_batch(_p(p), rsdims, _p(out), _p(ret), n)
    return ret, out


def rs_decode_word(word):
    d = np.ascontiguousarray(word, np.uint8).astype(np.uint32)
    assert d.size == 120
    rc = lib().ref_decode_rs(_p(d))
    return rc, d.astype(np.uint8)


def rs_decode_words(words):
    """(n, 120) uint8 -> (ret[n] int32, patched words (n, 120) uint8)"""
    d = np.ascontiguousarray(words, np.uint8).reshape(-1, 120).astype(np.uint32)
    ret = np.zeros(d.shape[0], np.int32)
    lib().ref_decode_rs_batch(_p(d), _p(ret), d.shape[0])
    return ret, d.astype(np.uint8)


def tables():
    ato = np.empty(768, np.uint8)
    iof = np.empty(256, np.uint8)
    lib().ref_tables(_p(ato), _p(iof))
    return ato, iof


if __name__ == "__main__":
    print("oracle/_ref:", "built" if build(force=True) else "no reference checkout, nothing built")
