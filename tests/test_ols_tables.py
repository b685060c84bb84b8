"""The overlap-save FIR's host tables (solid_dsp_amd/csrc/ols_tables.cpp), on the CPU.

tools/ols_tables_dump.cpp, built by the csrc Makefile with plain g++, writes the raw tables of one
case; three checks per case:

1. digests: SHA-256 of every table equals tests/golden/ols_tables_digests.json, recorded when
   the tables still were the loops of runtime.cpp's ols_build / ols_long_build (moved verbatim,
   before the spectrum's phase table): the arithmetic has not moved by a bit since;
2. exact packing identities between the tables of one case;
3. an independent restatement in numpy (np.fft.fft of g over N, exp(-2 pi j m / n) for the
   twiddles, the layouts written out again).  Two f64 routes can straddle an f32 rounding
   boundary, so per complex entry  |a - b| <= 2^-23 |b| + 1e-12 max|G|  (max|G| := 1 for the
   twiddle tables): one f32 rounding, plus a term far above the f64 sums' own error, which is of
   order L 2^-53 sum|g|.

Taps are white, as in test_gpu_fir_ols_white.py: default_rng(20251118).standard_normal(L) as f32
(CC32: an independent imaginary part), scale 0.2, on CC32 0.2 - 0.15j.
"""
import functools
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "solid_dsp_amd", "csrc")
DUMP = os.path.join(REPO, "solid_dsp_amd", "_build", "ols_tables_dump")
GOLDEN = os.path.join(REPO, "tests", "golden", "ols_tables_digests.json")

F32, C64, C128 = np.float32, np.complex64, np.complex128
RR32, RC32, CC32 = 0, 1, 2
TAP_SEED = 20251118
N = 4096
HALF_ROW = 257                      # kOlsHalfRow
TAB_CD, TAB_EF, TAB_F4 = 816, 1072, 1088  # kOlsOsTabCD, kOlsOsTabEF, kOlsOsTabF4

# (dtype, L, log2n); log2n = 0: the 4096-point tables
CASES = [(RR32, 2, 0), (RR32, 700, 0), (RC32, 256, 0), (RC32, 3841, 0), (CC32, 257, 0), (CC32, 3841, 0),
         (RC32, 3842, 14), (RC32, 3842, 13), (CC32, 3842, 14), (CC32, 3842, 13)]
SHORT = [c for c in CASES if c[2] == 0]
LONG = [c for c in CASES if c[2]]


def case_id(case):
    dtype, L, log2n = case
    return f"{('rr32', 'rc32', 'cc32')[dtype]}-L{L}" + (f"-log2n{log2n}" if log2n else "")


def white_taps(L, cplx):
    rng = np.random.default_rng(TAP_SEED)
    h = rng.standard_normal(L).astype(F32)
    if cplx:
        h = (h + 1j * rng.standard_normal(L).astype(F32)).astype(C64)
    return h


def coefs(case):
    """(stored taps, scale) in the handle's coefficient type"""
    dtype, L, _ = case
    if dtype == CC32:
        return white_taps(L, True), np.array([0.2 - 0.15j], dtype=C64)
    return white_taps(L, False), np.array([0.2], dtype=F32)


@functools.lru_cache(maxsize=None)
def dump_program():
    subprocess.run(["make", "-s", "-C", CSRC, "../_build/ols_tables_dump"], check=True)
    return DUMP


@functools.lru_cache(maxsize=None)
def tables(case):
    """{name: raw bytes} of one case, as the dump program wrote them"""
    dtype, _, log2n = case
    h, s = coefs(case)
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(s.tobytes() + h.tobytes())
        subprocess.run([dump_program(), str(dtype), str(log2n), src, dst], check=True, stderr=subprocess.DEVNULL)
        with open(dst, "rb") as f:
            raw = f.read()
    out, o = {}, 0
    while o < len(raw):
        name = raw[o:o + 8].rstrip(b"\0").decode()
        n = int.from_bytes(raw[o + 8:o + 16], "little")
        out[name] = raw[o + 16:o + 16 + n]
        o += 16 + n
    assert o == len(raw)
    return out


def c32(t, name):
    return np.frombuffer(t[name], dtype=C64)


def digests(case):
    return {k: hashlib.sha256(v).hexdigest() for k, v in tables(case).items()}


# ---------------------------------------------------------------- 1. digests
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_digests(case):
    with open(GOLDEN) as f:
        want = json.load(f)[case_id(case)]
    assert digests(case) == want


# ---------------------------------------------------------------- 2. exact identities
@pytest.mark.parametrize("case", SHORT, ids=case_id)
def test_packing_identities(case):
    t = tables(case)
    G = np.frombuffer(t["G"], dtype=C128)
    Gf = G.astype(C64)  # the tables' one rounding
    Hs, tw1, tw2 = c32(t, "Hs").reshape(256, 16), c32(t, "tw1").reshape(256, 16), c32(t, "tw2").reshape(16, 16)
    lane = np.arange(256)
    bins = (lane >> 4) + 16 * (lane & 15)  # k0 + 16 k1 of lane 16 k0 + k1
    assert np.array_equal(Hs, Gf[bins[:, None] + 256 * np.arange(16)[None, :]])

    pkt = c32(t, "pkt").reshape(4224, 2)  # one float4 = two c32
    for q in range(8):
        assert np.array_equal(pkt[q * 256:(q + 1) * 256], Hs[:, 2 * q:2 * q + 2])
        assert np.array_equal(pkt[2048 + q * 256:2048 + (q + 1) * 256], tw1[:, 2 * q:2 * q + 2])
        assert np.array_equal(pkt[4096 + q * 16:4096 + (q + 1) * 16], tw2[:, 2 * q:2 * q + 2])

    os_ = c32(t, "os").reshape(TAB_F4, 2)
    assert np.array_equal(os_[TAB_CD:TAB_CD + 256, 0], os_[0:256, 0])      # C1
    assert np.array_equal(os_[TAB_CD:TAB_CD + 256, 1], os_[256:512, 1])    # D1
    assert np.array_equal(os_[TAB_EF:TAB_EF + 16, 0], os_[768:784, 0])     # E1
    assert np.array_equal(os_[TAB_EF:TAB_EF + 16, 1], os_[784:800, 1])     # F1

    real_taps = case[0] == RC32
    assert ("hh" in t) == real_taps
    if real_taps:
        k = np.arange(1, N // 2)
        assert np.array_equal(G[N - k], np.conj(G[k]))
        assert G[0].imag == 0.0 and G[N // 2].imag == 0.0
        hh = c32(t, "hh").reshape(4, HALF_ROW, 2)
        for q in range(4):
            assert np.array_equal(hh[q, :256, 0], Gf[bins + 256 * (2 * q)])
            assert np.array_equal(hh[q, :256, 1], Gf[bins + 256 * (2 * q + 1)])
            # the mirror slot of lane (0, 0): the kernel's conj-and-swap yields bins 2p, 2p + 1, p = 7 - q
            p = 7 - q
            assert np.array_equal(np.conj(hh[q, 256, ::-1]), Gf[[256 * 2 * p, 256 * (2 * p + 1)]])


@pytest.mark.parametrize("case", LONG, ids=case_id)
def test_long_transpose(case):
    t = tables(case)
    log2n = case[2]
    N1, N2 = 1 << (log2n // 2), 1 << (log2n - log2n // 2)
    assert (N1 == N2) == (log2n == 14)
    lG, nat = c32(t, "lG").reshape(N1, N2), c32(t, "lGnat")
    k1, k2 = np.arange(N1)[:, None], np.arange(N2)[None, :]
    assert np.array_equal(lG, nat[k1 + N1 * k2])
    assert len(t["ltw"]) == 8 * (N1 + N2)


# ---------------------------------------------------------------- 3. numpy restatement
def close(a, b, gmax, what):
    a, b = np.asarray(a).astype(C128).ravel(), np.asarray(b).astype(C128).ravel()
    assert a.shape == b.shape, what
    over = np.abs(a - b) - (2.0 ** -23 * np.abs(b) + 1e-12 * gmax)
    assert over.max() <= 0.0, f"{what}: entry {int(over.argmax())} misses the bound by {over.max():.3e}"


def scaled_reversed(case):
    h, s = coefs(case)
    return h[::-1].astype(C128) * complex(s[0])


def W(n, m):
    return np.exp(-2j * np.pi * (np.asarray(m) % n) / n)


@pytest.mark.parametrize("case", SHORT, ids=case_id)
def test_numpy_restatement(case):
    t = tables(case)
    G = np.fft.fft(scaled_reversed(case), N) / N
    gmax = float(np.abs(G).max())
    close(np.frombuffer(t["G"], dtype=C128), G, gmax, "G")
    lane, col = np.arange(256)[:, None], np.arange(16)[None, :]
    Hs = G[(lane >> 4) + 16 * (lane & 15) + 256 * col]
    tw1, tw2 = W(4096, lane * col), W(256, np.arange(16)[:, None] * col)
    close(c32(t, "Hs"), Hs, gmax, "Hs")
    close(c32(t, "tw1"), tw1, 1.0, "tw1")
    close(c32(t, "tw2"), tw2, 1.0, "tw2")

    def pairs(rows):  # [q][i] = entries 2q, 2q + 1 of row i
        return rows.reshape(rows.shape[0], 8, 2).transpose(1, 0, 2)
    pkt = c32(t, "pkt").reshape(4224, 2)
    close(pkt[:2048], pairs(Hs), gmax, "pkt H")
    close(pkt[2048:4096], pairs(tw1), 1.0, "pkt tw1")
    close(pkt[4096:], pairs(tw2), 1.0, "pkt tw2")

    c, l = np.arange(256), np.arange(16)
    powers = [(1, 2), (3, 4), (8, 12)]
    os_ = np.concatenate([np.stack([W(4096, a * c), W(4096, b * c)], 1) for a, b in powers] +
                         [np.stack([W(256, a * l), W(256, b * l)], 1) for a, b in powers] +
                         [np.stack([W(4096, c), W(4096, 4 * c)], 1), np.stack([W(256, l), W(256, 4 * l)], 1)])
    close(c32(t, "os"), os_, 1.0, "os")

    if "hh" in t:
        hh = np.empty((4, HALF_ROW, 2), dtype=C128)
        for q in range(4):
            hh[q, :256] = Hs[:, 2 * q:2 * q + 2]
            # bins k2 = 15 - 2q and 14 - 2q of lane (0, 0), conjugated: those of k2' = 16 - k2 = 2q + 1, 2q + 2
            hh[q, 256] = G[[256 * (2 * q + 1), 256 * (2 * q + 2)]]
        close(c32(t, "hh"), hh, gmax, "hh")


@pytest.mark.parametrize("case", LONG, ids=case_id)
def test_numpy_restatement_long(case):
    t = tables(case)
    log2n = case[2]
    n, N1, N2 = 1 << log2n, 1 << (log2n // 2), 1 << (log2n - log2n // 2)
    G = np.fft.fft(scaled_reversed(case), n) / n
    gmax = float(np.abs(G).max())
    close(c32(t, "lG"), G.reshape(N2, N1).T, gmax, "lG")  # [k1][k2] = G[k1 + N1 k2]
    close(c32(t, "ltw"), np.concatenate([W(N1, np.arange(N1)), W(N2, np.arange(N2))]), 1.0, "ltw")


if __name__ == "__main__":  # the digests of this build, as the fixture holds them
    json.dump({case_id(c): digests(c) for c in CASES}, sys.stdout, indent=1, sort_keys=True)
    print()
