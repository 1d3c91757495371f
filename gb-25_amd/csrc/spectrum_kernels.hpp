// spectrum_kernels.hpp -- zonal wavenumber spectra (gb25_get_zonal_spectrum / gb25_get_derived_zonal_spectrum, include/gb25.h): the
// coefficients X(m) = A(m) - i B(m) of the direct transform along the grid's index i of every line (row j, level k) of a field or of
// a packed derived array.  Included by gb25_api.hip, launched from spectrum_host.hpp.
//
// The order of every sum is part of the ABI (numpy restates it bit for bit, gb-25_amd/spectra.py): A and B are SEQUENTIAL sums
// over i ascending from +0.0, every product and sum rounded to fp64, contraction OFF.  So LANES OWN WAVENUMBERS (the "lanes own
// bins" idiom of k_class_rows) and there is no reduction across lanes, no atomic on a floating-point number:
//   k_zonal_spectrum<T, TABLE_LDS>  a block of four waves takes LB = 4 lpw consecutive lines and the 64 wavenumbers of blockIdx.y.
//                     A wave's 64 lanes are lpw lines x mpad wavenumbers (mpad = the power of two >= min(m_count, 64), lpw =
//                     64 / mpad): a narrow window of wavenumbers fills the lanes with further lines.  The block walks i in chunks of
//                     ic columns: it stages the chunk of its LB lines as doubles in LDS (pitch odd: lanes of different lines read
//                     different banks; lanes of one line read one address, a broadcast) and notes a value that is not finite in
//                     the line's flag; then every lane walks the chunk upward: x(i) from LDS, the pair (cos, sin) of
//                     r = (m g) mod N from the interleaved table -- ONE 16-byte read --, two multiplies, two adds, and
//                     r += m, if (r >= N) r -= N.  r starts from (m global_offset_x) mod N computed in 64 bits.  A and B live in
//                     registers across the chunks.  A flagged line stores +0.0 for every coefficient and is counted once (an
//                     integer atomic by the lane of its first wavenumber in the blocks of blockIdx.y == 0).
//                     TABLE_LDS: the table (16 N bytes) is copied into LDS by every block; false: read from global memory where
//                     it does not fit -- the same values, the same bits.
//                     LDS, dynamic: 16 N (table) + 8 LB pitch (lines, <= 18 KB) + 4 LB (flags).
// Every offset into the source is a 64-bit element offset; plain vector loads and stores.
#pragma once

namespace gb25 {

constexpr int SPEC_THREADS = 256;
constexpr int SPEC_STAGE = 2048;   // doubles of line values a block stages per chunk (before the padding of the pitch)

struct SpecPair {   // one entry of the table: cos(2 pi r / N), sin(2 pi r / N)
  double c, s;
};
struct SpecCoef {   // = gb25_spectral_coefficient
  double re, im;
};
// the lines of the source: element (i, j, kk) at origin + kk plane + j pitch + i; line = kk by + j
struct SpecLines {
  long long origin, pitch, plane;
  int bx, by, kc;
};
// the window of wavenumbers and the shape of a block (spectrum_host.hpp, spec_shape)
struct SpecShape {
  int N, goff;            // columns of the GLOBAL grid; global 0-based column of local column 0
  int m_first, m_count;
  int mpad, mshift, lpw;  // lanes per line (1 << mshift), lines per wave
  int ic, xpitch;         // columns per chunk; doubles between two staged lines (odd)
};

template <class T, bool TABLE_LDS>
__global__ __launch_bounds__(SPEC_THREADS) void k_zonal_spectrum(const T* __restrict__ src, SpecLines L, SpecShape S,
                                                                 const SpecPair* __restrict__ table, SpecCoef* __restrict__ out,
                                                                 unsigned* __restrict__ bad_lines) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char spec_lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int LB = 4 * S.lpw;
  SpecPair* s_tab = (SpecPair*)spec_lds;
  double* s_x = (double*)(s_tab + (TABLE_LDS ? S.N : 0));
  int* s_bad = (int*)(s_x + LB * S.xpitch);
  const long long nlines = (long long)L.by * L.kc, line0 = (long long)blockIdx.x * LB;
  if (TABLE_LDS)
    for (int r = tid; r < S.N; r += SPEC_THREADS) s_tab[r] = table[r];
  for (int s = tid; s < LB; s += SPEC_THREADS) s_bad[s] = 0;
  // this lane's line and wavenumber; a lane beyond either computes on a valid one and stores nothing
  const int slot = w * S.lpw + (lane >> S.mshift);
  const int mi = (lane & (S.mpad - 1)) + 64 * (int)blockIdx.y;
  const bool live = mi < S.m_count && line0 + slot < nlines;
  const int mm = S.m_first + (mi < S.m_count ? mi : 0);
  int r = (int)(((long long)mm * S.goff) % S.N);
  double A = 0.0, B = 0.0;
  const double* xs = s_x + slot * S.xpitch;
  __syncthreads();
  for (int i0 = 0; i0 < L.bx; i0 += S.ic) {
    const int n = L.bx - i0 < S.ic ? L.bx - i0 : S.ic;
    for (int e = tid; e < LB * n; e += SPEC_THREADS) {
      const int s = e / n, c = e - s * n;
      const long long ln = line0 + s;
      double v = 0.0;
      if (ln < nlines) {
        const long long kk = ln / L.by, j = ln - kk * L.by;
        v = (double)src[L.origin + kk * L.plane + j * L.pitch + i0 + c];
        if (!__builtin_isfinite(v)) s_bad[s] = 1;
      }
      s_x[s * S.xpitch + c] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < n; c++) {
      const double x = xs[c];
      const SpecPair p = TABLE_LDS ? s_tab[r] : table[r];
      A = A + x * p.c;
      B = B + x * p.s;
      r += mm;
      if (r >= S.N) r -= S.N;
    }
    __syncthreads();
  }
  if (live) {
    const bool bad = s_bad[slot] != 0;
    SpecCoef o;
    o.re = bad ? 0.0 : A;
    o.im = bad ? 0.0 : -B;
    out[(line0 + slot) * S.m_count + mi] = o;
    if (bad && mi == 0) atomicAdd(bad_lines, 1u);
  }
}

}  // namespace gb25
