"""CPU-side checks of the synthesis channeliser's C-ABI boundary (sdsp_ichan_*, include/sdsp.h) and of
the numpy restatements its GPU tests stand on (tests/ichan_cases.py): the symbols are exported, create
refuses bad arguments in its documented order and a missing device before any device work, the
restatements agree with each other, and the inputs of tests/test_gpu_ichan.py can see the mistakes
they are there to catch.  No compute calls (the library has no CPU path)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import rel_rms
from ichan_cases import (C64, C128, F32, F64, chan_ref, check_streams, ichan_exact, ichan_f32, ichan_ref,
                         pair_identity, white_frames, white_taps)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "sdsp.h")

E_COEFFICIENTS_LENGTH_ZERO, E_NOT_ENOUGH_FILTERS = 1, 4
E_INVALID_ARGUMENT, E_UNSUPPORTED, E_NO_DEVICE = 90, 91, 101
NAMES = ("create", "destroy", "set_streams", "set_tuning", "reset", "channels", "subfilter_len", "execute_block",
         "execute_block_device", "info", "synchronize")


def ichan_symbols():
    text = open(HDR).read()
    return sorted(set(re.findall(r"SDSP_API\s+[\w\s\*]+?\b(sdsp_ichan_\w+)\s*\(", text)))


def test_header_declares_the_family():
    syms = ichan_symbols()
    assert syms == sorted("sdsp_ichan_" + n for n in NAMES)
    text = open(HDR).read()
    assert re.search(r"SDSP_TUNE_ICHAN_KERNEL\s*=\s*25\b", text)
    assert re.search(r"SDSP_TUNE_ICHAN_FRAMES_PER_BLOCK\s*=\s*26\b", text)
    assert re.search(r"SDSP_API\s+size_t\s+sdsp_ichan_channels\s*\(\s*const\s+sdsp_ichan\s*\*", text)
    assert re.search(r"SDSP_API\s+size_t\s+sdsp_ichan_subfilter_len\s*\(\s*const\s+sdsp_ichan\s*\*", text)


def test_library_exports_and_python_binds_every_symbol():
    import solid_dsp_amd as sd
    out = subprocess.run(["nm", "-D", "--defined-only", sd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sdsp_\w+)", out))
    missing = [s for s in ichan_symbols() if s not in exported]
    assert not missing, missing
    lib = sd.lib()
    for s in ichan_symbols():
        assert getattr(lib, s).argtypes is not None, s  # declared by _lib, not merely found
    assert sd.ChannelSynthesizer is sd.synthesizer.ChannelSynthesizer
    assert (sd._lib.TUNE_ICHAN_KERNEL, sd._lib.TUNE_ICHAN_FRAMES_PER_BLOCK) == (25, 26)


def _create(lib, dtype, len_, M, device=0, null_taps=False, coef_dt=np.float32):
    taps = np.ones(max(len_, 1), dtype=coef_dt)
    h = C.c_void_p(0xdead)  # create must null it on every failure
    p = None if null_taps else taps.ctypes.data_as(C.c_void_p)
    rc = lib.sdsp_ichan_create(C.byref(h), dtype, p, len_, M, device)
    return rc, h


def _message(lib):
    m = lib.sdsp_last_error()
    return m.decode() if isinstance(m, bytes) else (m or "")


def test_create_refuses_bad_arguments_in_order():
    """every argument check comes before the device check, so this holds with and without a GPU; each
    call breaks one more rule than the check it expects to fire, so the order shows"""
    import solid_dsp_amd as sd
    lib = sd.lib()
    # 1. null out (with everything else wrong too)
    assert lib.sdsp_ichan_create(None, -1, None, 16, 0, 0) == E_INVALID_ARGUMENT
    for dtype in (-1, sd.RR32, sd.CC32, sd.RR64, sd.CC64, 6):  # 2. dtype, ahead of null taps and channels = 0
        rc, h = _create(lib, dtype, 16, 0, null_taps=True)
        assert rc == E_UNSUPPORTED and not h.value, dtype
        assert "SDSP_RC32" in _message(lib)
    rc, h = _create(lib, sd.RC32, 16, 0, null_taps=True)  # 3. null taps with len > 0, ahead of channels = 0
    assert rc == E_INVALID_ARGUMENT and not h.value
    assert "null" in _message(lib)
    rc, h = _create(lib, sd.RC32, 0, 0)  # 4. channels = 0, ahead of len = 0
    assert rc == E_NOT_ENOUGH_FILTERS and not h.value
    assert "NotEnoughFilters" in _message(lib)
    rc, h = _create(lib, sd.RC64, 0, 3, null_taps=True, coef_dt=np.float64)  # 5. len = 0 (null taps are fine then),
    assert rc == E_COEFFICIENTS_LENGTH_ZERO and not h.value                  # ahead of channels = 3
    assert "CoefficientsLengthZero" in _message(lib)
    for M in (1, 2, 3, 12, 1000, 8192, 1 << 20):  # 6. not a power of two in [4, 4096], ahead of len < channels
        rc, h = _create(lib, sd.RC32, 1, M)
        assert rc == E_UNSUPPORTED and not h.value, M
        assert "power of two" in _message(lib)
    for M, n in ((4, 3), (64, 63), (4096, 4095)):  # 7. len < channels
        rc, h = _create(lib, sd.RC32, n, M)
        assert rc == E_INVALID_ARGUMENT and not h.value, (M, n)
        assert "fewer taps" in _message(lib)


def test_no_device_fails_loudly():
    import solid_dsp_amd as sd
    lib = sd.lib()
    if sd.device_count() > 0:
        rc, h = _create(lib, sd.RC32, 16, 8, device=sd.device_count() + 7)
    else:
        rc, h = _create(lib, sd.RC32, 16, 8)
        with pytest.raises(sd.SdspError) as e:
            sd.ChannelSynthesizer(np.ones(16, dtype=np.float32), 8)
        assert e.value.code == E_NO_DEVICE
    assert rc == E_NO_DEVICE and not h.value  # no CPU fallback


def test_null_handle_calls():
    import solid_dsp_amd as sd
    lib = sd.lib()
    assert lib.sdsp_ichan_channels(None) == 0
    assert lib.sdsp_ichan_subfilter_len(None) == 0
    sz, k = C.c_size_t(77), C.c_int(0)
    for call in (lambda: lib.sdsp_ichan_reset(None), lambda: lib.sdsp_ichan_set_streams(None, 2),
                 lambda: lib.sdsp_ichan_set_tuning(None, 25, 1), lambda: lib.sdsp_ichan_set_tuning(None, 26, 8),
                 lambda: lib.sdsp_ichan_info(None, C.byref(k), C.byref(sz)),
                 lambda: lib.sdsp_ichan_synchronize(None),
                 lambda: lib.sdsp_ichan_execute_block(None, None, 0, None, C.byref(sz)),
                 lambda: lib.sdsp_ichan_execute_block_device(None, None, 0, None, C.byref(sz), None)):
        assert call() == E_INVALID_ARGUMENT
    lib.sdsp_ichan_destroy(None)  # a no-op


# ---------------------------------------------------------------- the restatements
@pytest.mark.parametrize("M,Kh,Kg", [(4, 1, 1), (8, 3, 2), (64, 5, 8)])
def test_pair_identity(M, Kh, Kg):
    """ichan_ref(g, M, chan_ref(h, M, x)) equals the closed form, white taps and a white stream, 1e-12"""
    frames = 20
    h, g = white_taps(M * Kh, C128), white_taps(M * Kg, C128, seed=7)
    x = O.synth(5, 0, 0, M * frames, complex_=True).astype(C128)
    y = ichan_ref(g, M, chan_ref(h, M, x, C128), C128)
    rel = rel_rms(y, pair_identity(g, h, M, x, C128))
    print(f"pair identity M={M} K_h={Kh} K_g={Kg}: rel-RMS {rel:.3e}")
    assert rel <= 1e-12


@pytest.mark.parametrize("M", [4, 64])
def test_ones_taps_give_m_x(M):
    """K = 1 and all-ones taps on both sides: y = M x"""
    x = O.synth(6, 0, 0, M * 9, complex_=True).astype(C128)
    ones = np.ones(M)
    y = ichan_ref(ones, M, chan_ref(ones, M, x, C128), C128)
    assert rel_rms(y, M * x) <= 1e-12


@pytest.mark.parametrize("M,K", [(8, 1), (8, 5), (64, 3)])
@pytest.mark.parametrize("prec", [C64, C128], ids=["c64", "c128"])
def test_exact_restatement_is_the_definition(M, K, prec):
    """ichan_exact on numpy's own inverse transforms (rounded to the precision) against ichan_ref: the
    same sums, so they agree to the precision's rounding; and the taps' tail is ignored by both"""
    frames = 11
    g = white_taps(M * K + 3, prec)
    X = white_frames(1, frames, M, prec)[0]
    U = np.concatenate([np.zeros((K - 1, M), prec), (np.fft.ifft(X.astype(C128), axis=1) * M).astype(prec)])
    y = ichan_exact(g, M, U, prec)
    assert y.dtype == prec and y.shape == (frames * M,)
    assert rel_rms(y, ichan_ref(g, M, X, prec)) <= (5e-7 if prec == C64 else 1e-15)
    assert np.array_equal(y, ichan_exact(g[:M * K], M, U, prec))


@pytest.mark.parametrize("M,K", [(64, 8), (1024, 8)])
def test_what_the_inputs_see(M, K):
    """with white taps and white frames a reversed tap vector and a missing M-1-r flip each move ichan_ref
    by more than 0.5 rel-RMS (measured 1.17 to 1.43); with symmetric Kaiser taps the reversal is
    invisible, which is why every GPU case uses white taps"""
    frames = 45
    X = white_frames(1, frames, M)[0]
    g = white_taps(M * K)
    ref = ichan_ref(g, M, X)
    reversed_taps = rel_rms(ichan_ref(g[::-1].copy(), M, X), ref)
    no_flip = rel_rms(ichan_ref(g, M, X, flip=False), ref)
    print(f"M={M} K={K} white taps: reversed taps move the output by {reversed_taps:.3f} rel-RMS, "
          f"a missing flip by {no_flip:.3f}")
    assert reversed_taps > 0.5 and no_flip > 0.5
    kaiser = O.firdes_kaiser(M * K, 0.5 / M, 80.0, 0.0).astype(F32)
    # a symmetric design read backwards is the same design
    assert rel_rms(ichan_ref(kaiser[::-1].copy(), M, X), ichan_ref(kaiser, M, X)) <= 1e-12


@pytest.mark.parametrize("K", [1, 8, 12])
@pytest.mark.parametrize("M", [4, 64, 1024, 4096])
def test_f32_arithmetic_alone_stays_inside(M, K):
    """f32 branch sums behind a single-precision inverse FFT on the CPU, white taps and frames, 45 frames:
    both criteria of check_streams at half the GPU limit"""
    frames = 45
    g = white_taps(M * K)
    X = white_frames(1, frames, M)[0]
    check_streams(ichan_f32(g, M, X)[None], ichan_ref(g, M, X)[None], M, 5e-7, f"f32 on the CPU M={M} K={K}")
