"""The arbitrary-rate resampler's definition (include/sdsp.h, sdsp_arb_*) restated on the host, for
tests/test_arb_capi.py (on the oracle alone) and tests/test_gpu_arb.py (on the device
interpolator's output).  Everything here is integer arithmetic on Python ints or uint64 arrays, plus
the one formula a + mu (c - a) applied in the sample's dtype on real views, so every operation is
rounded once."""
import numpy as np

ONE = 1 << 32
MASK = ONE - 1
STEP_MIN, STEP_MAX = 1 << 16, 1 << 48
RATES = [0.9187512345, 1.0000123, 2.718281828, 0.1234567]


def step_of(rate):
    """sdsp_arb_step_from_rate in Python doubles"""
    return int(np.floor(np.ldexp(1.0 / rate, 32) + 0.5))


def count(step, t, n):
    """(n_out, next_t): the closed form of the definition, on Python ints"""
    end = n * ONE
    if t >= end:
        return 0, t - end
    n_out = -(-(end - t) // step)
    return n_out, t + n_out * step - end


def walk(step, t, n):
    """(n_out, next_t) by brute force: one output per step while the time is inside the call"""
    end = n * ONE
    emitted = 0
    while t < end:
        emitted += 1
        t += step
    return emitted, t - end


def select(step, t, n_out, P):
    """(u, m) per output: u = j P + b, the interpolated sample c sits on, counted from the call's
    first input; m the 32 fraction bits mu is made of"""
    k = np.arange(n_out, dtype=np.uint64)
    T = np.uint64(t) + k * np.uint64(step)  # < 2^63
    j, f = T >> np.uint64(32), T & np.uint64(MASK)
    v = f * np.uint64(P)  # P < 2^31
    b, m = v >> np.uint64(32), v & np.uint64(MASK)
    return (j * np.uint64(P) + b).astype(np.int64), m


def lerp(z, z_prev, u, m):
    """out[k] = a + mu (c - a), a = z(u - 1), c = z(u), z(-1) = z_prev, in z's dtype on real views:
    the subtraction, the product and the addition are each rounded once (numpy does not fuse)"""
    z = np.asarray(z)
    rdt = z.real.dtype.type
    zz = np.concatenate([np.asarray([z_prev], dtype=z.dtype), z])  # zz[i + 1] = z(i)
    a, c = zz[u], zz[u + 1]
    mu = m.astype(rdt) * rdt(2.0 ** -32)  # round to nearest, then an exact scaling
    if z.dtype.kind == "c":
        ar, cr = a.view(rdt).reshape(-1, 2), c.view(rdt).reshape(-1, 2)
        out = ar + mu[:, None] * (cr - ar)
        return np.ascontiguousarray(out).view(z.dtype).reshape(-1)
    return a + mu * (c - a)


def model(z, z_prev, step, t, n, P, flip_mu=False):
    """one call on the interpolated stream z of its n inputs: (out, next_t).  flip_mu is one of
    the mistakes tests/test_arb_capi.py tries: 1 - mu in place of mu"""
    n_out, nxt = count(step, t, n)
    u, m = select(step, t, n_out, P)
    if flip_mu:
        m = (np.uint64(ONE) - m) & np.uint64(MASK)
    return lerp(z, z_prev, u, m), nxt
