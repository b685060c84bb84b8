// Host-only tables of the overlap-save FIR kernels: pure functions of the taps, the scale and the
// transform size (layouts: ols_tables.cpp).  No HIP runtime call, no handle: runtime.cpp (FirOls)
// uploads what they return, tools/ols_tables_dump.cpp writes it out for tests/test_ols_tables.py.
// `taps`: L stored coefficients of `dtype` (sdsp_dtype), `scale`: one; g[i] = scale * h[L-1-i].
#pragma once
#include <vector>

#include "sdsp_host.hpp"

namespace sdsp {

// real taps and a real scale on complex samples: exactly conjugate-symmetric spectrum, half table
bool ols_real_taps(int dtype, const unsigned char* scale);
// G[k], k < 4096: the spectrum of g over N = 4096, divided by N, in f64
std::vector<cd> ols_spectrum(const unsigned char* taps, const unsigned char* scale, int dtype, size_t L);
// lane rows, c32: Hs [256][16] = G[k0 + 16 k1 + 256 k2] of row t = 16 k0 + k1; [rows][16] =
// Wn^(t k): tw1 = (256, 4096), tw2 = (16, 256); pkt: the three k-pair major (4224 float4)
std::vector<float> ols_rows_H(const std::vector<cd>& G);
std::vector<float> ols_rows_tw(int rows, int n);
std::vector<float> ols_pack_pkt(const std::vector<float>& Hs, const std::vector<float>& tw1,
                                const std::vector<float>& tw2);
std::vector<float> ols_os_bases();                         // one-shot kernel's twiddle bases (kOlsOsTabF4 float4)
std::vector<float> ols_half_table(const std::vector<cd>& G);  // ols_real_taps: 4 * kOlsHalfRow float4
// long path, N = 2^log2n = N1 N2, N1 = 2^(log2n / 2): the spectrum of g over N, divided by N, c32
// in [k1][k2] order (k = k1 + N1 k2); the tables [N1 | N2], c32 e^{-j 2 pi m / N1}, e^{-j 2 pi m / N2}
std::vector<float> ols_long_spectrum(const unsigned char* taps, const unsigned char* scale, int dtype, size_t L,
                                     int log2n);
std::vector<float> ols_long_twiddles(int log2n);

}  // namespace sdsp
