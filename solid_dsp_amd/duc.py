"""Digital up-converter on MI355X: ``NCO`` mix-up fused into ``InterpolatingFIRFilter``.

A build-defined composition of two reference objects (src/filter/fir/interp.rs,
src/nco/mod.rs), as the down-converter and the channeliser are: ``DUC(taps, M)``
with an oscillator ``(theta, delta_theta)`` computes, sample for sample,

    y = interpolator.execute(x[j])
    for p in 0..M: out[j*M + p] = nco.mix_up(y[p]); nco.step()

in one pass (``kern_duc.hip``): the interpolated stream is never written to
memory.  ``ALGO_EXACT`` is bit-identical to an ``ALGO_EXACT``
``InterpolatingFIRFilter`` followed by ``NCO.mix_block_device(down=False)``;
``ALGO_FMA`` sums with fused multiply-adds.  Samples are complex (complex64 /
complex128); taps real or complex of the same precision.  There is no scale (the
interpolator has none).  A block object: there is no per-sample ``execute``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _handle as H
from . import _lib as L


class DUC(H.Oscillator, H.FirHandle):
    _family = "duc"

    def __init__(self, taps, interpolation=1, sample_dtype=None, coef_dtype=None, device=0, channels=1, algo=None):
        c = self._coefs(taps, sample_dtype, coef_dtype)
        h = C.c_void_p()
        L.check(L.lib().sdsp_duc_create(C.byref(h), self.dtype, L.ptr(c), len(c), int(interpolation), int(device)))
        self._adopt(h, device, channels, algo)  # algo None: ALGO_FMA when the process default is, else ALGO_EXACT

    @classmethod
    def new(cls, taps, interpolation, **kw):
        return cls(taps, interpolation, **kw)

    # ---- configuration -------------------------------------------------
    set_channels, get_algo = H.set_channels, H.get_algo
    set_algo = H.set_algo  # ALGO_EXACT or ALGO_FMA

    def set_direction(self, down: bool):
        """False (default): mix_up; True: mix_down."""
        self._call("set_direction", 1 if down else 0)

    def interpolation(self) -> int:
        return int(L.lib().sdsp_duc_interpolation(self._h))

    def subfilter_len(self) -> int:
        return int(L.lib().sdsp_duc_subfilter_len(self._h))

    # ---- blocks ----------------------------------------------------------
    def execute_block(self, samples) -> np.ndarray:
        """Host samples (channel-major [channels, n] when channels > 1) -> n * M mixed outputs
        per channel."""
        x, n = self._block_in(samples)
        y = self._block_out(n * self.interpolation())
        if n:
            L.check(L.lib().sdsp_duc_execute_block(self._h, L.ptr(x), n, L.ptr(y)))
        return y

    def execute_block_device(self, d_in, n: int, d_out, stream=None) -> int:
        """Device-resident block: d_in / d_out are torch tensors or raw device pointers
        (channel-major, n samples per channel in, n * M per channel out)."""
        m = self.interpolation()
        pin = L.device_ptr(d_in, self.sample_dtype, self.channels * n, self.device, "input")
        pout = L.device_ptr(d_out, self.sample_dtype, self.channels * n * m, self.device, "output")
        L.check(L.lib().sdsp_duc_execute_block_device(self._h, pin, n, pout, L.stream_handle(stream)))
        return n * m
