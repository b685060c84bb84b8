// Tables of the overlap-save FIR kernels, one function per layout (ols_tables.hpp).  The
// kernels' bits follow every rounding here: the twiddles are cos(-2.0 * M_PI * m / n) (put_w),
// the spectrum's phases cos(w * p) with w = -2.0 * M_PI / N, and the two are not the same doubles.
#include "ols_tables.hpp"

#include <cmath>

#include "sdsp_kernels.hpp"

namespace sdsp {

namespace {
// g[i] = scale * h[L-1-i]
cd scaled_tap(const unsigned char* taps, int dtype, size_t L, cd s, size_t i) {
    const cd c = coef_at(taps, dtype, L - 1 - i);
    return coef_is_complex(dtype) ? cmul(c, s) : cd{c.re * s.re, c.re * s.im};
}
void put_c(std::vector<float>& v, size_t i, cd x) {
    v[2 * i] = (float)x.re;
    v[2 * i + 1] = (float)x.im;
}
// v[i] = e^{-j 2 pi m / n} as c32 (m < n)
void put_w(std::vector<float>& v, size_t i, long long m, size_t n) {
    const double ang = -2.0 * M_PI * (double)m / (double)n;
    put_c(v, i, cd{std::cos(ang), std::sin(ang)});
}
}  // namespace

bool ols_real_taps(int dtype, const unsigned char* scale) {
    return !coef_is_complex(dtype) && !(dtype == SDSP_RR32) && coef_at(scale, dtype, 0).im == 0.0;
}

std::vector<cd> ols_spectrum(const unsigned char* taps, const unsigned char* scale, int dtype, size_t L) {
    const int N = kOlsN;
    std::vector<cd> g(L);
    const cd s = coef_at(scale, dtype, 0);
    for (size_t i = 0; i < L; ++i) g[i] = scaled_tap(taps, dtype, L, s, i);
    // direct DFT in f64 (O(N L) per build); the phase w * ph takes N values, tabulated once
    std::vector<cd> G(N);
    const double w = -2.0 * M_PI / N;
    std::vector<double> cs(N), sn_(N);
    for (int p = 0; p < N; ++p) {
        cs[p] = std::cos(w * (double)p);
        sn_[p] = std::sin(w * (double)p);
    }
    for (int k = 0; k < N; ++k) {
        double re = 0.0, im = 0.0;
        for (size_t i = 0; i < L; ++i) {
            const long long ph = ((long long)i * k) % N;
            const double c = cs[ph], sn = sn_[ph];
            re += g[i].re * c - g[i].im * sn;
            im += g[i].re * sn + g[i].im * c;
        }
        G[k] = {re / N, im / N};
    }
    // real taps, real scale, complex samples: g is real, so its spectrum is conjugate-symmetric.
    // The sums above are so only to rounding; the symmetry is made exact here, before anything is
    // rounded to f32 or packed, so that the full tables and the half table hold the same values
    // and every kernel computes the same bits from either (kern_fir_ols_os.hip REALG)
    if (ols_real_taps(dtype, scale)) {
        for (int k = 1; k < N / 2; ++k) G[N - k] = cd{G[k].re, -G[k].im};
        G[0].im = 0.0;
        G[N / 2].im = 0.0;
    }
    return G;
}

std::vector<float> ols_rows_H(const std::vector<cd>& G) {
    std::vector<float> Hs(2 * 4096);
    for (int t = 0; t < 256; ++t) {
        const int k0 = t >> 4, k1 = t & 15;
        for (int k2 = 0; k2 < 16; ++k2) put_c(Hs, t * 16 + k2, G[k0 + 16 * k1 + 256 * k2]);
    }
    return Hs;
}

std::vector<float> ols_rows_tw(int rows, int n) {
    std::vector<float> tw(2 * 16 * rows);
    for (int t = 0; t < rows; ++t)
        for (int k = 0; k < 16; ++k) put_w(tw, t * 16 + k, (t * k) % n, n);
    return tw;
}

// k-pair major so that a table load is one coalesced 16-byte access per lane: float4 (p, i) =
// entries 2p, 2p + 1 of row i; [0, 2048): H rows t, [2048, 4096): tw1 rows, [4096, 4224): tw2 rows
std::vector<float> ols_pack_pkt(const std::vector<float>& Hs, const std::vector<float>& tw1,
                                const std::vector<float>& tw2) {
    std::vector<float> pkt(4 * 4224);
    auto pack = [&](int f4, const std::vector<float>& rows, int n) {  // n rows of 16 c32
        for (int q = 0; q < 8; ++q)
            for (int i = 0; i < n; ++i)
                for (int e = 0; e < 4; ++e) pkt[4 * (f4 + q * n + i) + e] = rows[2 * (i * 16 + 2 * q) + e];
    };
    pack(0, Hs, 256);
    pack(2048, tw1, 256);
    pack(4096, tw2, 16);
    return pkt;
}

// per column c the twiddle bases C_b = W4096^(b c), D_a = W4096^(4 a c) (b, a = 1..3) as float4
// [q][c] = (C1 C2 | C3 D1 | D2 D3), then per row l the W256 bases E_b = W256^(b l),
// F_a = W256^(4 a l) as float4 [768 + 16 q + l], then the first powers alone (kOlsOsTabCD,
// kOlsOsTabEF: the default kernel's two loads)
std::vector<float> ols_os_bases() {
    std::vector<float> os(4 * kOlsOsTabF4);
    static const int pw[3][2] = {{1, 2}, {3, 4}, {8, 12}};
    for (int q = 0; q < 3; ++q)
        for (int h = 0; h < 2; ++h) {
            for (int c = 0; c < 256; ++c) put_w(os, 2 * (256 * q + c) + h, (pw[q][h] * c) % 4096, 4096);
            for (int l = 0; l < 16; ++l) put_w(os, 2 * (768 + 16 * q + l) + h, (pw[q][h] * l) % 256, 256);
        }
    for (int c = 0; c < 256; ++c) {  // {C1, D1} per column
        put_w(os, 2 * (kOlsOsTabCD + c), c, 4096);
        put_w(os, 2 * (kOlsOsTabCD + c) + 1, (4 * c) % 4096, 4096);
    }
    for (int l = 0; l < 16; ++l) {  // {E1, F1} per row
        put_w(os, 2 * (kOlsOsTabEF + l), l, 256);
        put_w(os, 2 * (kOlsOsTabEF + l) + 1, (4 * l) % 256, 256);
    }
    return os;
}

// real taps: H[N - k] = conj(H[k]), so the one-shot kernel reads bins k2 < 8 of every lane from
// a half table and the others as the conjugates of its mirror lane's (kern_fir_ols_os.hip):
// float4 [p][i] = {H(i, 2p), H(i, 2p + 1)} for p < 4, H(i, k2) = G[k0 + 16 k1 + 256 k2] of
// lane i = 16 k0 + k1; entry i = 256 is the mirror of lane (0, 0), whose bins k2 >= 8 mirror
// k2' = 16 - k2 (k2' = 8 included): stored so that the kernel's conj-and-swap yields them
std::vector<float> ols_half_table(const std::vector<cd>& G) {
    std::vector<float> hh(4 * 4 * kOlsHalfRow);
    auto set = [&](int q, int i, int half, cd v) { put_c(hh, 2 * (q * kOlsHalfRow + i) + half, v); };
    for (int q = 0; q < 4; ++q) {
        for (int i = 0; i < 256; ++i)
            for (int half = 0; half < 2; ++half) set(q, i, half, G[(i >> 4) + 16 * (i & 15) + 256 * (2 * q + half)]);
        // lane (0, 0), pair p = 7 - q of its bins k2 = 2p, 2p + 1: stored as
        // {conj H(256 (2p + 1)), conj H(256 (2p))} at the mirror slot
        const int pp = 7 - q;
        const cd a = G[256 * (2 * pp + 1)], b = G[256 * (2 * pp)];
        set(q, 256, 0, cd{a.re, -a.im});
        set(q, 256, 1, cd{b.re, -b.im});
    }
    return hh;
}

std::vector<float> ols_long_spectrum(const unsigned char* taps, const unsigned char* scale, int dtype, size_t L,
                                     int log2n) {
    const int l1 = log2n / 2, l2 = log2n - l1;
    const size_t N = (size_t)1 << log2n, N1 = (size_t)1 << l1, N2 = (size_t)1 << l2;
    std::vector<double> g(2 * N, 0.0);
    const cd s = coef_at(scale, dtype, 0);
    for (size_t i = 0; i < L; ++i) {
        const cd v = scaled_tap(taps, dtype, L, s, i);
        g[2 * i] = v.re;
        g[2 * i + 1] = v.im;
    }
    host_fft_pow2(g, N);
    std::vector<float> G(2 * N);
    for (size_t k1 = 0; k1 < N1; ++k1)
        for (size_t k2 = 0; k2 < N2; ++k2) {
            const size_t k = k1 + N1 * k2, o = k1 * N2 + k2;
            put_c(G, o, cd{g[2 * k] / (double)N, g[2 * k + 1] / (double)N});
        }
    return G;
}

std::vector<float> ols_long_twiddles(int log2n) {
    const size_t N1 = (size_t)1 << (log2n / 2), N2 = (size_t)1 << (log2n - log2n / 2);
    std::vector<float> tw(2 * (N1 + N2));
    for (size_t m = 0; m < N1; ++m) put_w(tw, m, m, N1);
    for (size_t m = 0; m < N2; ++m) put_w(tw, N1 + m, m, N2);
    return tw;
}

}  // namespace sdsp
