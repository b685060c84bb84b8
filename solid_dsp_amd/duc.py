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

from . import _lib as L
from .filter.fir import _coef_array, _default_sample


class DUC:
    def __init__(self, taps, interpolation=1, sample_dtype=None, coef_dtype=None, device=0, channels=1, algo=None):
        c = _coef_array(taps, coef_dtype)
        if sample_dtype is None:
            sample_dtype = _default_sample(c.dtype)
        self.dtype = L.dtype_code(c.dtype, sample_dtype)
        self.coef_dtype = L.COEF_DTYPE[self.dtype]
        self.sample_dtype = L.SAMPLE_DTYPE[self.dtype]
        h = C.c_void_p()
        L.check(L.lib().sdsp_duc_create(C.byref(h), self.dtype, L.ptr(c), len(c), int(interpolation), int(device)))
        self._h = h
        self.device = device
        self.channels = 1
        if channels != 1:
            self.set_channels(channels)
        if algo is not None:  # default: ALGO_FMA when the process default is, else ALGO_EXACT
            self.set_algo(algo)

    @classmethod
    def new(cls, taps, interpolation, **kw):
        return cls(taps, interpolation, **kw)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            L.lib().sdsp_duc_destroy(h)
            self._h = None

    # ---- configuration -------------------------------------------------
    def set_channels(self, channels: int):
        L.check(L.lib().sdsp_duc_set_channels(self._h, channels))
        self.channels = channels

    def set_algo(self, algo: int):
        """ALGO_EXACT or ALGO_FMA"""
        L.check(L.lib().sdsp_duc_set_algo(self._h, int(algo)))

    def get_algo(self) -> int:
        return int(L.lib().sdsp_duc_get_algo(self._h))

    def set_direction(self, down: bool):
        """False (default): mix_up; True: mix_down."""
        L.check(L.lib().sdsp_duc_set_direction(self._h, 1 if down else 0))

    def interpolation(self) -> int:
        return int(L.lib().sdsp_duc_interpolation(self._h))

    def subfilter_len(self) -> int:
        return int(L.lib().sdsp_duc_subfilter_len(self._h))

    def clone(self):
        h = C.c_void_p()
        L.check(L.lib().sdsp_duc_clone(self._h, C.byref(h)))
        obj = type(self).__new__(type(self))
        obj.__dict__.update({k: v for k, v in self.__dict__.items() if k != "_h"})
        obj._h = h
        return obj

    __copy__ = clone

    def reset(self):
        L.check(L.lib().sdsp_duc_reset(self._h))

    # ---- oscillator (NCO setters, src/nco/mod.rs:59-86) -----------------
    def set_frequency(self, delta_theta: float):
        L.check(L.lib().sdsp_duc_set_frequency(self._h, float(delta_theta)))

    def adjust_frequency(self, dt: float):
        L.check(L.lib().sdsp_duc_adjust_frequency(self._h, float(dt)))

    def set_phase(self, phi: float):
        L.check(L.lib().sdsp_duc_set_phase(self._h, float(phi)))

    def adjust_phase(self, delta_phi: float):
        L.check(L.lib().sdsp_duc_adjust_phase(self._h, float(delta_phi)))

    def nco_state(self):
        """(theta, delta_theta), the raw u32 registers"""
        th, dt = C.c_uint32(), C.c_uint32()
        L.check(L.lib().sdsp_duc_get_nco_state(self._h, C.byref(th), C.byref(dt)))
        return th.value, dt.value

    def set_nco_state(self, theta: int, delta_theta: int):
        L.check(L.lib().sdsp_duc_set_nco_state(self._h, int(theta) & 0xFFFFFFFF, int(delta_theta) & 0xFFFFFFFF))

    # ---- blocks ----------------------------------------------------------
    def execute_block(self, samples) -> np.ndarray:
        """Host samples (channel-major [channels, n] when channels > 1) -> n * M mixed outputs
        per channel."""
        x = np.ascontiguousarray(samples, dtype=self.sample_dtype)
        if self.channels > 1 and (x.ndim != 2 or x.shape[0] != self.channels):
            raise ValueError("multi-channel input must be [channels, n]")
        n = x.shape[-1] if x.ndim else 0
        m = self.interpolation()
        y = np.zeros((self.channels, n * m) if self.channels > 1 else n * m, dtype=self.sample_dtype)
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

    def synchronize(self):
        L.check(L.lib().sdsp_duc_synchronize(self._h))
