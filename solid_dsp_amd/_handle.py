"""What the classes that own a libsdsp.so handle share.

``Handle`` is the base of every such class: ``self._h`` is the handle and
``_family`` names its functions in the C ABI (``sdsp_<family>_*``,
include/sdsp.h).  ``FirHandle`` adds what the streaming FIR family has in
common (``_FirBase``, ``PolyPhaseFilterBank``, ``DDC``, ``DUC``, ``Resampler``):
clone, reset, synchronize, the constructor's dtype prologue and the host block
marshalling.  The configuration methods that only some of these classes have
(``set_channels``, ``set_algo``, ``get_algo``, ``set_tuning``, ``info``) are
written once below and bound by the classes whose C family has the function, and
the NCO setters of the two converters come from ``Oscillator``.  ``ChanHandle``
is the base of the three channelisers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def coef_array(coefs, coef_dtype):
    a = np.asarray(coefs)
    if coef_dtype is None:
        coef_dtype = a.dtype if a.dtype in (np.float32, np.float64, np.complex64, np.complex128) else np.float64
    return np.ascontiguousarray(a, dtype=coef_dtype)


def default_sample(coef_dtype):
    return {np.dtype(np.float32): np.complex64, np.dtype(np.float64): np.complex128,
            np.dtype(np.complex64): np.complex64, np.dtype(np.complex128): np.complex128}[np.dtype(coef_dtype)]


class Handle:
    _family = None  # "fir", "pfb", "ddc", ...

    def _call(self, name, *args):
        """sdsp_<family>_<name>(handle, *args), a non-zero status raised"""
        L.check(getattr(L.lib(), f"sdsp_{self._family}_{name}")(self._h, *args))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            getattr(L.lib(), f"sdsp_{self._family}_destroy")(h)
            self._h = None


class FirHandle(Handle):
    def _coefs(self, coefs, sample_dtype, coef_dtype):
        """The constructor prologue: the contiguous coefficient array; sets dtype (the sdsp_dtype
        pair), coef_dtype and sample_dtype."""
        c = coef_array(coefs, coef_dtype)
        if sample_dtype is None:
            sample_dtype = default_sample(c.dtype)
        self.dtype = L.dtype_code(c.dtype, sample_dtype)
        self.coef_dtype = L.COEF_DTYPE[self.dtype]
        self.sample_dtype = L.SAMPLE_DTYPE[self.dtype]
        return c

    def _adopt(self, h, device, channels, algo):
        """After create: take the handle, then the channels, then the algorithm (None: the
        handle's own start, sdsp.h)."""
        self._h = h
        self.device = device
        self.channels = 1
        if channels != 1:
            self.set_channels(channels)
        if algo is not None:
            self.set_algo(algo)

    def clone(self):
        h = C.c_void_p()
        self._call("clone", C.byref(h))
        obj = type(self).__new__(type(self))
        obj.__dict__.update(self.__dict__)  # whatever a subclass added travels
        obj._h = h
        return obj

    __copy__ = clone

    def reset(self):
        self._call("reset")

    def synchronize(self):
        self._call("synchronize")

    # ---- host blocks ------------------------------------------------------
    def _block_in(self, samples):
        """(x, n): the samples as a contiguous array of the handle's sample dtype, [n] or
        channel-major [channels, n]"""
        x = np.ascontiguousarray(samples, dtype=self.sample_dtype)
        if self.channels > 1 and (x.ndim != 2 or x.shape[0] != self.channels):
            raise ValueError("multi-channel input must be [channels, n]")
        return x, (x.shape[-1] if x.ndim else 0)

    def _block_out(self, n_out):
        """zeros [n_out], or [channels, n_out] when channels > 1"""
        return np.zeros((self.channels, n_out) if self.channels > 1 else n_out, dtype=self.sample_dtype)


# ---- configuration, for the classes whose family has the function ------------
def set_channels(self, channels: int):
    """zeroes the delay lines, and the block phase where the family has one"""
    self._call("set_channels", channels)
    self.channels = channels


def set_algo(self, algo: int):
    """ALGO_* (include/sdsp.h says which the family takes)"""
    self._call("set_algo", int(algo))


def get_algo(self) -> int:
    return int(getattr(L.lib(), f"sdsp_{self._family}_get_algo")(self._h))


def set_tuning(self, key: int, value: int):
    """kernel-variant knobs (SDSP_TUNE_*, include/sdsp.h): performance only"""
    self._call("set_tuning", int(key), int(value))


def info(self):
    """(kernel, frames_per_block): the kernel the next call runs (the class's KERNELS) and its frames
    per workgroup on a long block"""
    k, f = C.c_int(), C.c_size_t()
    self._call("info", C.byref(k), C.byref(f))
    return k.value, f.value


class ChanHandle(Handle):
    """The channeliser family (``Channelizer``, ``ChannelSynthesizer``, ``OversampledChannelizer``): M
    channels, real taps and complex samples, one frame every ``_step`` time samples (M, or D)."""

    def _create(self, taps, channels, sample_dtype, device, streams, *stride):
        """sdsp_<family>_create(&h, dtype, taps, len, channels, *stride, device), then the streams"""
        self.dtype = L.RC32 if np.dtype(sample_dtype) == np.complex64 else L.RC64
        self.coef_dtype = L.COEF_DTYPE[self.dtype]
        self.sample_dtype = L.SAMPLE_DTYPE[self.dtype]
        t = np.ascontiguousarray(taps, dtype=self.coef_dtype)
        h = C.c_void_p()
        L.check(getattr(L.lib(), f"sdsp_{self._family}_create")(
            C.byref(h), self.dtype, L.ptr(t) if len(t) else None, len(t), channels, *stride, device))
        self._h = h
        self.M = channels
        self._step = stride[0] if stride else channels
        self.device = device
        self.streams = 1
        if streams != 1:
            self.set_streams(streams)

    set_tuning = set_tuning

    def set_streams(self, streams: int):
        """zeroes the history and the frame phase"""
        self._call("set_streams", streams)
        self.streams = streams

    def reset(self):
        self._call("reset")

    def synchronize(self):
        self._call("synchronize")

    def execute_block_device(self, d_in, n: int, d_out, stream=None) -> int:
        """Device-resident block of n = frames * step samples per stream: [streams, n] time samples
        and [streams, frames, M] channel samples, whichever way the family goes.  Returns the frame
        count."""
        fr = C.c_size_t(0)
        pin = L.device_ptr(d_in, self.sample_dtype, self.streams * n, self.device, "input")
        pout = L.device_ptr(d_out, self.sample_dtype, self.streams * (n // self._step) * self.M, self.device,
                            "output")
        self._call("execute_block_device", pin, n, pout, C.byref(fr), L.stream_handle(stream))
        return fr.value


class Oscillator:
    """The NCO setters of a converter (src/nco/mod.rs:59-86) and its raw registers."""

    def set_frequency(self, delta_theta: float):
        self._call("set_frequency", float(delta_theta))

    def adjust_frequency(self, dt: float):
        self._call("adjust_frequency", float(dt))

    def set_phase(self, phi: float):
        self._call("set_phase", float(phi))

    def adjust_phase(self, delta_phi: float):
        self._call("adjust_phase", float(delta_phi))

    def nco_state(self):
        """(theta, delta_theta), the raw u32 registers"""
        th, dt = C.c_uint32(), C.c_uint32()
        self._call("get_nco_state", C.byref(th), C.byref(dt))
        return th.value, dt.value

    def set_nco_state(self, theta: int, delta_theta: int):
        self._call("set_nco_state", int(theta) & 0xFFFFFFFF, int(delta_theta) & 0xFFFFFFFF)
