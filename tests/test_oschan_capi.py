"""CPU-side checks of the oversampled channeliser's C-ABI boundary (sdsp_oschan_*, include/sdsp.h) and of
the numpy restatements its GPU tests stand on (tests/oschan_cases.py): the symbols are exported, create
refuses bad arguments in its documented order and a missing device before any device work, the
restatements agree with each other, and the inputs of tests/test_gpu_oschan.py can see the mistakes
they are there to catch.  No compute calls (the library has no CPU path)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_util import rel_rms
from ichan_cases import chan_ref
from oschan_cases import (C64, C128, FRAMES, check_streams, ddc_form, ddc_taps, hist_len, oschan_exact, oschan_f32,
                          oschan_ref, oschan_split, white_streams, white_taps)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "sdsp.h")

E_COEFFICIENTS_LENGTH_ZERO, E_NOT_ENOUGH_FILTERS = 1, 4
E_INVALID_ARGUMENT, E_UNSUPPORTED, E_NO_DEVICE = 90, 91, 101
NAMES = ("create", "destroy", "set_streams", "set_tuning", "reset", "channels", "decimation", "subfilter_len",
         "phase", "execute_block", "execute_block_device", "info", "synchronize")
SIX = [(8, 3, 8), (8, 3, 6), (8, 3, 1), (64, 5, 48), (16, 1, 4), (16, 2, 5)]  # (M, K, D)


def oschan_symbols():
    text = open(HDR).read()
    return sorted(set(re.findall(r"SDSP_API\s+[\w\s\*]+?\b(sdsp_oschan_\w+)\s*\(", text)))


def test_header_declares_the_family():
    assert len(NAMES) == 13
    assert oschan_symbols() == sorted("sdsp_oschan_" + n for n in NAMES)
    text = open(HDR).read()
    assert re.search(r"SDSP_TUNE_OSCHAN_KERNEL\s*=\s*27\b", text)
    assert re.search(r"SDSP_TUNE_OSCHAN_FRAMES_PER_BLOCK\s*=\s*28\b", text)
    for getter in ("channels", "decimation", "subfilter_len", "phase"):
        assert re.search(rf"SDSP_API\s+size_t\s+sdsp_oschan_{getter}\s*\(\s*const\s+sdsp_oschan\s*\*", text), getter


def test_library_exports_and_python_binds_every_symbol():
    import solid_dsp_amd as sd
    out = subprocess.run(["nm", "-D", "--defined-only", sd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (sdsp_\w+)", out))
    missing = [s for s in oschan_symbols() if s not in exported]
    assert not missing, missing
    lib = sd.lib()
    for s in oschan_symbols():
        assert getattr(lib, s).argtypes is not None, s  # declared by _lib, not merely found
    assert sd.OversampledChannelizer is sd.oschan.OversampledChannelizer
    assert (sd._lib.TUNE_OSCHAN_KERNEL, sd._lib.TUNE_OSCHAN_FRAMES_PER_BLOCK) == (27, 28)


def _create(lib, dtype, len_, M, D, device=0, null_taps=False, coef_dt=np.float32):
    taps = np.ones(max(len_, 1), dtype=coef_dt)
    h = C.c_void_p(0xdead)  # create must null it on every failure
    p = None if null_taps else taps.ctypes.data_as(C.c_void_p)
    rc = lib.sdsp_oschan_create(C.byref(h), dtype, p, len_, M, D, device)
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
    assert lib.sdsp_oschan_create(None, -1, None, 16, 0, 0, 0) == E_INVALID_ARGUMENT
    for dtype in (-1, sd.RR32, sd.CC32, sd.RR64, sd.CC64, 6):  # 2. dtype, ahead of null taps and channels = 0
        rc, h = _create(lib, dtype, 16, 0, 0, null_taps=True)
        assert rc == E_UNSUPPORTED and not h.value, dtype
        assert "SDSP_RC32" in _message(lib)
    rc, h = _create(lib, sd.RC32, 16, 0, 0, null_taps=True)  # 3. null taps with len > 0, ahead of channels = 0
    assert rc == E_INVALID_ARGUMENT and not h.value
    assert "null" in _message(lib)
    rc, h = _create(lib, sd.RC32, 0, 0, 0)  # 4. channels = 0, ahead of len = 0
    assert rc == E_NOT_ENOUGH_FILTERS and not h.value
    assert "NotEnoughFilters" in _message(lib)
    rc, h = _create(lib, sd.RC64, 0, 3, 0, null_taps=True, coef_dt=np.float64)  # 5. len = 0 (null taps are fine
    assert rc == E_COEFFICIENTS_LENGTH_ZERO and not h.value                     # then), ahead of channels = 3
    assert "CoefficientsLengthZero" in _message(lib)
    for M in (1, 2, 3, 12, 1000, 8192, 1 << 20):  # 6. not a power of two in [4, 4096], ahead of decimation = 0
        rc, h = _create(lib, sd.RC32, 1, M, 0)
        assert rc == E_UNSUPPORTED and not h.value, M
        assert "power of two" in _message(lib)
    for M, D in ((4, 0), (4, 5), (64, 65), (4096, 1 << 40)):  # 7. decimation = 0 or > channels, ahead of len < channels
        rc, h = _create(lib, sd.RC32, M - 1, M, D)
        assert rc == E_UNSUPPORTED and not h.value, (M, D)
        assert "decimation" in _message(lib)
    for M, n, D in ((4, 3, 4), (64, 63, 1), (4096, 4095, 3000)):  # 8. len < channels
        rc, h = _create(lib, sd.RC32, n, M, D)
        assert rc == E_INVALID_ARGUMENT and not h.value, (M, n)
        assert "fewer taps" in _message(lib)


def test_no_device_fails_loudly():
    import solid_dsp_amd as sd
    lib = sd.lib()
    if sd.device_count() > 0:
        rc, h = _create(lib, sd.RC32, 16, 8, 6, device=sd.device_count() + 7)
    else:
        rc, h = _create(lib, sd.RC32, 16, 8, 6)
        with pytest.raises(sd.SdspError) as e:
            sd.OversampledChannelizer(np.ones(16, dtype=np.float32), 8, 6)
        assert e.value.code == E_NO_DEVICE
    assert rc == E_NO_DEVICE and not h.value  # no CPU fallback


def test_null_handle_calls():
    import solid_dsp_amd as sd
    lib = sd.lib()
    for getter in (lib.sdsp_oschan_channels, lib.sdsp_oschan_decimation, lib.sdsp_oschan_subfilter_len,
                   lib.sdsp_oschan_phase):
        assert getter(None) == 0
    sz, k = C.c_size_t(77), C.c_int(0)
    for call in (lambda: lib.sdsp_oschan_reset(None), lambda: lib.sdsp_oschan_set_streams(None, 2),
                 lambda: lib.sdsp_oschan_set_tuning(None, 27, 1), lambda: lib.sdsp_oschan_set_tuning(None, 28, 8),
                 lambda: lib.sdsp_oschan_info(None, C.byref(k), C.byref(sz)),
                 lambda: lib.sdsp_oschan_synchronize(None),
                 lambda: lib.sdsp_oschan_execute_block(None, None, 0, None, C.byref(sz)),
                 lambda: lib.sdsp_oschan_execute_block_device(None, None, 0, None, C.byref(sz), None)):
        assert call() == E_INVALID_ARGUMENT
    lib.sdsp_oschan_destroy(None)  # a no-op


# ---------------------------------------------------------------- the restatements
@pytest.mark.parametrize("M,K", [(4, 1), (8, 3), (64, 5)])
@pytest.mark.parametrize("prec", [C64, C128], ids=["c64", "c128"])
def test_critically_sampled_is_the_channeliser(M, K, prec):
    """D = M: the rotation is 0 and the output is chan_ref's, difference 0.0"""
    h = white_taps(M * K + 3, prec)
    x = white_streams(1, M * 20, prec)[0]
    assert np.array_equal(oschan_ref(h, M, M, x, prec), chan_ref(h, M, x, prec))


@pytest.mark.parametrize("M,K,D", SIX)
def test_every_channel_is_a_down_converter(M, K, D):
    """oschan_ref equals the mix / convolve / decimate form, 1e-10 relative"""
    h = white_taps(M * K, C128)
    x = white_streams(1, D * FRAMES, C128)[0]
    rel = rel_rms(oschan_ref(h, M, D, x, C128), ddc_form(h, M, D, x, C128))
    print(f"ddc form M={M} K={K} D={D}: rel-RMS {rel:.3e}")
    assert rel <= 1e-10


def test_ddc_form_is_a_convolution():
    """ddc_form forms only the kept outputs; np.convolve's full output, decimated, is the same"""
    M, K, D = 8, 3, 6
    h = white_taps(M * K, C128)
    x = white_streams(1, D * 20, C128)[0].astype(C128)
    g, n = ddc_taps(h, M, C128), np.arange(len(x))
    for k in (0, 1, 5):
        full = np.convolve(x * np.exp(2j * np.pi * k * (n + 1) / M), g)[D - 1::D][:20]
        assert rel_rms(ddc_form(h, M, D, x, C128, channels=[k])[:, 0], full) <= 1e-12


@pytest.mark.parametrize("M,K,D", SIX)
def test_split_restatement_is_the_whole_stream(M, K, D):
    """oschan_ref call by call, with the frame index and the history carried, equals one call exactly;
    and the taps' tail is ignored"""
    h = white_taps(M * K + 3)
    x = white_streams(1, D * FRAMES)[0]
    whole = oschan_ref(h, M, D, x)
    assert np.array_equal(oschan_split(h, M, D, x, [1, 2, 8, 34]), whole)
    assert np.array_equal(oschan_ref(h[:M * K], M, D, x), whole)


@pytest.mark.parametrize("M,K,D", [(8, 1, 8), (8, 3, 5), (64, 5, 48)])
@pytest.mark.parametrize("prec", [C64, C128], ids=["c64", "c128"])
def test_exact_restatement_is_the_definition(M, K, D, prec):
    """numpy's FFT of oschan_exact's frames against oschan_ref: the same sums, so they agree to the
    precision's rounding; a later first frame index rotates as oschan_ref does"""
    h = white_taps(M * K, prec)
    x = white_streams(1, D * 11, prec)[0]
    xh = np.concatenate([np.zeros(hist_len(M, K, D), prec), x])
    for m0 in (0, 7):
        w = oschan_exact(h, M, D, xh, m0, prec)
        assert w.dtype == prec and w.shape == (11, M)
        assert rel_rms(np.fft.fft(w.astype(C128), axis=1), oschan_ref(h, M, D, x, prec, m0)) <= \
            (5e-7 if prec == C64 else 1e-15)


@pytest.mark.parametrize("M,K,D", [(4, 1, 1), (4, 12, 3), (64, 8, 48), (64, 8, 32), (1024, 8, 512), (1024, 12, 768),
                                   (4096, 8, 2048), (4096, 1, 4096)])
def test_f32_arithmetic_alone_stays_inside(M, K, D):
    """f32 branch sums behind a single-precision FFT on the CPU, white taps and a white stream, 45 frames:
    both criteria of check_streams at half the GPU limit"""
    h = white_taps(M * K)
    x = white_streams(1, D * FRAMES)[0]
    check_streams(oschan_f32(h, M, D, x).reshape(1, -1), oschan_ref(h, M, D, x).reshape(1, -1), M, 5e-7,
                  f"f32 on the CPU M={M} K={K} D={D}")


@pytest.mark.parametrize("M,K,D", [(8, 3, 6), (64, 8, 48), (1024, 3, 1000), (16, 5, 1)])
def test_what_the_inputs_see(M, K, D):
    """with white taps and a white stream, 45 frames, four mistakes each move oschan_ref by more than 0.5
    rel-RMS: no rotation, a rotation of the opposite sign, a rotation by m D instead of (m+1) D, and a
    frame counter restarted at a second call after 7 frames.  Two blind spots, which the GPU cases
    avoid: at D = M/2 the wrong sign moves the output by exactly 0, and a restart after a frame count
    with frames D = 0 (mod M) is invisible"""
    h = white_taps(M * K)
    x = white_streams(1, D * FRAMES)[0]
    ref = oschan_ref(h, M, D, x)
    moved = {
        "no rotation": rel_rms(oschan_ref(h, M, D, x, shift=lambda m: 0), ref),
        "opposite sign": rel_rms(oschan_ref(h, M, D, x, shift=lambda m: -(m + 1) * D), ref),
        "m D": rel_rms(oschan_ref(h, M, D, x, shift=lambda m: m * D), ref),
        "restart after 7": rel_rms(oschan_split(h, M, D, x, [7, FRAMES - 7], restart=True), ref),
    }
    print(f"M={M} K={K} D={D}: " + ", ".join(f"{k} {v:.3f}" for k, v in moved.items()))
    for k, v in moved.items():
        assert v > 0.5, (k, v)
    # the blind spots
    xh = white_streams(1, (M // 2) * FRAMES)[0]
    assert np.array_equal(oschan_ref(h, M, M // 2, xh, shift=lambda m: -(m + 1) * (M // 2)),
                          oschan_ref(h, M, M // 2, xh))
    assert np.array_equal(oschan_split(h, M, M // 2, xh, [8, FRAMES - 8], restart=True), oschan_ref(h, M, M // 2, xh))
