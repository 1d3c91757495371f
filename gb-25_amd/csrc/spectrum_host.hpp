// spectrum_host.hpp -- host side of gb25_get_spectrum_table / gb25_get_zonal_spectrum / gb25_get_derived_zonal_spectrum /
// gb25_spectral_coefficient_bytes (include/gb25.h); included by gb25_api.hip behind diagnostics_host.hpp, whose shared helpers
// (diag_*) and sources (DiagSource: a spectrum weighs with no measure, so every source has one, the vorticity too) it uses.
// Kernel: spectrum_kernels.hpp; the memory: spectrum (a result buffer), spec_* of DiagState (diagnostics_state.hpp).  Like the other diagnostics nothing here writes model memory or a schedule flag: the only memory
// written is the records' own buffer.
#pragma once

namespace {

static_assert(sizeof(SpecCoef) == sizeof(gb25_spectral_coefficient), "a record is a gb25_spectral_coefficient");
constexpr size_t SPEC_LDS_LIMIT = 160 * 1024;
constexpr size_t SPEC_HEAD = 16;   // bytes in front of the records: the count of the lines that were skipped

inline int spectrum_columns(const gb25_model* m) { return m->Nx * m->Rx; }   // N: the columns of the GLOBAL grid

// THE table of the definition: c[r] = cos((2 pi r) / N), s[r] likewise, every operation rounded to fp64, cos and sin of the host's
// libm.  A pure function of r and N: gb25_get_spectrum_table evaluates it for the caller, spectrum_table for the device.
inline void spectrum_entry(size_t r, size_t N, double* c, double* s) {
  const double a = (6.283185307179586 * (double)r) / (double)N;
  *c = std::cos(a);
  *s = std::sin(a);
}
// its interleaved copy on the device, once per model (and again after a rebuild of the grid)
gb25_status spectrum_table(gb25_model* m) {
  DiagState& D = m->diag;
  if (D.spec_valid) return GB25_OK;
  D.drop(D.spec_table);
  const size_t N = (size_t)spectrum_columns(m);
  std::vector<double> cs(2 * N);
  for (size_t r = 0; r < N; r++) spectrum_entry(r, N, &cs[2 * r], &cs[2 * r + 1]);
  if (gb25_status s = diag_upload(m, cs, &D.spec_table)) return s;
  D.spec_valid = true;
  return GB25_OK;
}

// how a block is cut (spectrum_kernels.hpp): lanes per line, lines per wave, columns per chunk
SpecShape spectrum_shape(const gb25_model* m, int m_first, int mc, int bx) {
  SpecShape S = {};
  S.N = spectrum_columns(m);
  S.goff = m->rx * m->Nx;
  S.m_first = m_first;
  S.m_count = mc;
  S.mpad = 1;
  while (S.mpad < mc && S.mpad < 64) S.mpad <<= 1, S.mshift++;
  S.lpw = 64 / S.mpad;
  S.ic = std::min(bx, SPEC_STAGE / (4 * S.lpw));
  S.xpitch = S.ic | 1;
  return S;
}

// What the sources share once they lie on the device: the buffer (the count, then the coefficients), the table, the launch, the
// copies.
gb25_status spectrum_run(gb25_model* m, const char* what, const real* src, const SpecLines& L, int m_first, int mc,
                         gb25_spectral_coefficient* out, int64_t* nonfinite_lines) {
  const size_t records = (size_t)L.by * L.kc * mc;
  if (gb25_status s = m->diag.spectrum.grow(m, what, "the coefficients", SPEC_HEAD + records * sizeof(SpecCoef))) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = spectrum_table(m)) return s;
  const SpecShape S = spectrum_shape(m, m_first, mc, L.bx);
  const int LB = 4 * S.lpw;
  const size_t stage = (size_t)LB * S.xpitch * sizeof(double) + (size_t)LB * sizeof(int), tab = (size_t)S.N * sizeof(SpecPair);
  const bool in_lds = m->spectrum_table_where != 1 && tab + stage <= SPEC_LDS_LIMIT;
  const size_t lds = stage + (in_lds ? tab : 0);
  auto kern = in_lds ? k_zonal_spectrum<real, true> : k_zonal_spectrum<real, false>;
  // (a function attribute is set per device: the flag lives in the model, not in the process)
  if (lds > 64 * 1024 && !m->diag.spec_lds_raised) {
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SPEC_LDS_LIMIT));
    m->diag.spec_lds_raised = true;
  }
  unsigned* bad = (unsigned*)m->diag.spectrum.p;
  SpecCoef* rec = (SpecCoef*)((char*)m->diag.spectrum.p + SPEC_HEAD);
  const long long nlines = (long long)L.by * L.kc;
  HIPCHK(hipMemsetAsync(bad, 0, SPEC_HEAD, m->stream));
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    const dim3 grd((unsigned)((nlines + LB - 1) / LB), (unsigned)((mc + 63) / 64));
    hipLaunchKernelGGL(kern, grd, dim3(SPEC_THREADS), lds, m->stream, src, L, S, (const SpecPair*)m->diag.spec_table, rec, bad);
    LAUNCHCHK();
  }
  // (the count lands in a word of the model: no copy is ever pending into a frame that has returned)
  HIPCHK(hipMemcpyAsync(&m->diag.spec_skipped, bad, sizeof m->diag.spec_skipped, hipMemcpyDeviceToHost, m->stream));
  if (gb25_status s = diag_download(m, out, rec, records * sizeof(SpecCoef))) return s;
  if (nonfinite_lines) *nonfinite_lines = (int64_t)m->diag.spec_skipped;
  return GB25_OK;
}

// the windows of wavenumbers and of levels, and the count they make; *mc, *kc: their lengths
gb25_status spectrum_windows(gb25_model* m, const char* what, int32_t m_first, int32_t m_count, int32_t k_first, int32_t k_count, int rows,
                             int levels, int64_t count, int* mc, int* kc) {
  if (gb25_status s = diag_window(m, what, m_first, m_count, spectrum_columns(m) / 2 + 1, "wavenumbers (m_first, m_count)", mc)) return s;
  if (gb25_status s = diag_window(m, what, k_first, k_count, levels, "levels (k_first, k_count)", kc)) return s;
  const int64_t want = (int64_t)*kc * rows * *mc;
  if (count != want)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: these windows have %lld records (levels %d, rows %d, wavenumbers %d), count is %lld", what,
                (long long)want, *kc, rows, *mc, (long long)count);
  return GB25_OK;
}

// the windows over the source's own rows and levels, the source, the launch (its plan P: the entry points make it, each where
// its checks have always stood)
gb25_status spectrum_of(gb25_model* m, const char* what, const DiagSource& S, const SourcePlan& P, int32_t m_first, int32_t m_count,
                        int32_t k_first, int32_t k_count, gb25_spectral_coefficient* out, int64_t count, int64_t* nonfinite_lines) {
  int mc = 0, kc = 0;
  if (gb25_status s = spectrum_windows(m, what, m_first, m_count, k_first, k_count, P.dims[1], P.dims[2], count, &mc, &kc)) return s;
  if (gb25_status s = diag_need_device(m, what)) return s;
  const real* src = nullptr;
  DiagBox b;
  if (gb25_status s = diag_source_resolve(m, S, P, k_first, kc, &src, &b)) return s;
  const SpecLines L = {b.origin, b.pitch, b.plane, b.bx, b.by, kc};
  return spectrum_run(m, what, src, L, m_first, mc, out, nonfinite_lines);
}

}  // namespace

extern "C" {

int32_t gb25_spectral_coefficient_bytes(void) { return (int32_t)sizeof(gb25_spectral_coefficient); }

gb25_status gb25_get_spectrum_table(const gb25_model* m, double* cos_out, double* sin_out, int64_t count) {
  // (read-only: nothing of the model is written, not even its error text)
  if (!m || !cos_out || !sin_out || count != (int64_t)spectrum_columns(m)) return GB25_ERR_INVALID_ARGUMENT;
  for (int64_t r = 0; r < count; r++) spectrum_entry((size_t)r, (size_t)count, &cos_out[r], &sin_out[r]);
  return GB25_OK;
}

gb25_status gb25_get_zonal_spectrum(gb25_model* m, gb25_field f, int32_t m_first, int32_t m_count, int32_t k_first, int32_t k_count,
                                    gb25_spectral_coefficient* out, int64_t count, int64_t* nonfinite_lines) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_get_zonal_spectrum";
  const DiagSource S(f);
  SourcePlan P;
  if (gb25_status s = diag_source_plan(m, what, S, &P)) return s;
  if (!out) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: out is NULL", what);
  int32_t d[3];
  if (gb25_field_dims(m, f, 0, d)) return GB25_ERR_INVALID_ARGUMENT;   // (a handle without a device has no fields: refused as ever, without a text)
  return spectrum_of(m, what, S, P, m_first, m_count, k_first, k_count, out, count, nonfinite_lines);
}

gb25_status gb25_get_derived_zonal_spectrum(gb25_model* m, gb25_derived q, double param, int32_t m_first, int32_t m_count,
                                            int32_t k_first, int32_t k_count, gb25_spectral_coefficient* out, int64_t count,
                                            int64_t* nonfinite_lines) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  const char* what = "gb25_get_derived_zonal_spectrum";
  if (!out) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: out is NULL", what);
  const DiagSource S(q, param);
  SourcePlan P;
  if (gb25_status s = diag_source_plan(m, what, S, &P)) return s;
  return spectrum_of(m, what, S, P, m_first, m_count, k_first, k_count, out, count, nonfinite_lines);
}

}  // extern "C"
