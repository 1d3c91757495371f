// classes_host.hpp -- host side of gb25_get_class_sums / gb25_class_sum_bytes (include/gb25.h); included by gb25_api.hip behind
// diagnostics_host.hpp, whose shared helpers (diag_*) and tables (moments_tables, diag_measure_tables) it uses.  Kernels:
// class_kernels.hpp; the memory: class_sums (a result buffer) of DiagState (diagnostics_state.hpp).  Like the other diagnostics nothing here writes model memory or a schedule
// flag: the only memory written is the records' own buffer.
#pragma once

namespace {

static_assert(sizeof(ClassPartial) == sizeof(gb25_class_sum), "a class record is a gb25_class_sum");
static_assert(CLASS_MAX_BINS == GB25_CLASS_MAX_BINS, "the kernels' cap is the header's");

// the edges (CLASS_MAX_BINS doubles), then ROWS [rows B], CUMULATIVE [rows (B + 1)] and TOTAL [B] of the call's B bins, each with
// room for the tallest set of rows a call can ask for (v below a wall: Ny + 1)
inline size_t class_max_rows(const gb25_model* m) { return (size_t)m->Ny + 1; }
gb25_status class_buffer(gb25_model* m, const char* what, int B) {
  const size_t records = class_max_rows(m) * (2 * (size_t)B + 1) + (size_t)B;
  return m->diag.class_sums.grow(m, what, "the class records", CLASS_MAX_BINS * sizeof(double) + records * sizeof(ClassPartial));
}
inline double* class_edges(gb25_model* m) { return (double*)m->diag.class_sums.p; }
inline ClassPartial* class_rows(gb25_model* m) { return (ClassPartial*)(class_edges(m) + CLASS_MAX_BINS); }
inline ClassPartial* class_psi(gb25_model* m, int B) { return class_rows(m) + class_max_rows(m) * (size_t)B; }
inline ClassPartial* class_total(gb25_model* m, int B) { return class_psi(m, B) + class_max_rows(m) * ((size_t)B + 1); }

struct ClassLaunch {
  const real *v, *T, *S;
  int i0, bx, N, B;
};
template <int WHAT, bool CURV>
void class_launch_var(gb25_model* m, const ClassTables& tab, int variable, const ClassLaunch& a) {
  const dim3 grd((unsigned)a.N), blk(CLASS_THREADS);
  ClassPartial* rows = class_rows(m);
  switch (variable) {
    case GB25_CLASS_T:
      hipLaunchKernelGGL((k_class_rows<WHAT, CURV, CLV_T>), grd, blk, 0, m->stream, m->g, tab, a.v, a.T, a.S, a.i0, a.bx, a.B, rows);
      break;
    case GB25_CLASS_S:
      hipLaunchKernelGGL((k_class_rows<WHAT, CURV, CLV_S>), grd, blk, 0, m->stream, m->g, tab, a.v, a.T, a.S, a.i0, a.bx, a.B, rows);
      break;
    default:
      hipLaunchKernelGGL((k_class_rows<WHAT, CURV, CLV_SIGMA>), grd, blk, 0, m->stream, m->g, tab, a.v, a.T, a.S, a.i0, a.bx, a.B, rows);
      break;
  }
}

}  // namespace

extern "C" {

int32_t gb25_class_sum_bytes(void) { return (int32_t)sizeof(gb25_class_sum); }

gb25_status gb25_get_class_sums(gb25_model* m, gb25_class_what what, gb25_class_variable variable, const double* edges,
                                int32_t n_edges, gb25_class_shape shape, int32_t i_first, int32_t i_count, gb25_class_sum* out,
                                int64_t count) {
  if (!m || !out || !edges) return GB25_ERR_INVALID_ARGUMENT;
  if (what != GB25_CL_FACES_Y && what != GB25_CL_CELLS)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_class_sums: what must be GB25_CL_FACES_Y or GB25_CL_CELLS, got %d", (int)what);
  if (variable != GB25_CLASS_T && variable != GB25_CLASS_S && variable != GB25_CLASS_POTENTIAL_DENSITY)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_class_sums: variable must be GB25_CLASS_T, GB25_CLASS_S or GB25_CLASS_POTENTIAL_DENSITY, got %d", (int)variable);
  if (shape != GB25_CL_ROWS && shape != GB25_CL_ROWS_CUMULATIVE && shape != GB25_CL_TOTAL)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_class_sums: shape must be GB25_CL_ROWS, GB25_CL_ROWS_CUMULATIVE or GB25_CL_TOTAL, got %d", (int)shape);
  if (n_edges < 1 || n_edges > GB25_CLASS_MAX_BINS - 1)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_class_sums: n_edges = %d, must be 1 .. %d (%d bins at the most)", (int)n_edges,
                GB25_CLASS_MAX_BINS - 1, GB25_CLASS_MAX_BINS);
  for (int e = 0; e < n_edges; e++)
    if (!std::isfinite(edges[e]) || (e > 0 && !(edges[e] > edges[e - 1])))
      return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_class_sums: the edges must be finite and strictly increasing (edge %d is %g)", e, edges[e]);
  const bool faces = what == GB25_CL_FACES_Y;
  int32_t d[3];
  if (gb25_field_dims(m, faces ? GB25_V : GB25_T, 0, d)) return GB25_ERR_INVALID_ARGUMENT;
  const int N = d[1], along = d[0], B = n_edges + 1;
  int n = 0;
  if (gb25_status s = diag_window(m, "gb25_get_class_sums", i_first, i_count, along, "columns (i_first, i_count)", &n)) return s;
  const int64_t want = shape == GB25_CL_ROWS ? (int64_t)N * B : shape == GB25_CL_ROWS_CUMULATIVE ? (int64_t)N * (B + 1) : (int64_t)B;
  if (count != want)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_get_class_sums: this shape has %lld records (rows %d, bins %d), count is %lld",
                (long long)want, N, B, (long long)count);
  if (gb25_status s = diag_need_device(m, "gb25_get_class_sums")) return s;
  ClassLaunch a = {nullptr, nullptr, nullptr, (int)i_first, n, N, B};
  if (faces)
    if (gb25_status s = diag_source(m, GB25_V, &a.v)) return s;
  if (gb25_status s = diag_source(m, GB25_T, &a.T)) return s;
  if (gb25_status s = diag_source(m, GB25_S, &a.S)) return s;
  if (gb25_status s = class_buffer(m, "gb25_get_class_sums", B)) return s;
  if ((size_t)N > class_max_rows(m)) return fail(m, GB25_ERR_STATE, "gb25_get_class_sums: more rows than the model's buffer holds");
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = moments_tables(m)) return s;
  double padded[CLASS_MAX_BINS];   // (alive until the stream is synchronised below)
  for (int e = 0; e < CLASS_MAX_BINS; e++) padded[e] = e < n_edges ? edges[e] : HUGE_VAL;
  HIPCHK(hipMemcpyAsync(class_edges(m), padded, sizeof padded, hipMemcpyHostToDevice, m->stream));
  const MomentsTables measure = diag_measure_tables(m, !faces);
  const ClassTables tab = {faces ? m->diag.face_length[0] : measure.area[0], measure.first[faces ? 2 : 0], m->diag.eos0, class_edges(m),
                           measure.pivot_row};
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    if (faces) {
      if (m->g.cv.on) class_launch_var<CL_FACES_Y, true>(m, tab, (int)variable, a);
      else class_launch_var<CL_FACES_Y, false>(m, tab, (int)variable, a);
    } else {
      if (m->g.cv.on) class_launch_var<CL_CELLS, true>(m, tab, (int)variable, a);
      else class_launch_var<CL_CELLS, false>(m, tab, (int)variable, a);
    }
    LAUNCHCHK();
    if (shape != GB25_CL_ROWS) {
      const int most = std::max(N, B);
      hipLaunchKernelGGL(k_class_fold, dim3((most + 63) / 64), dim3(64), 0, m->stream, (const ClassPartial*)class_rows(m), N, B,
                         class_psi(m, B), class_total(m, B));
      LAUNCHCHK();
    }
  }
  const ClassPartial* from = shape == GB25_CL_ROWS ? class_rows(m) : shape == GB25_CL_ROWS_CUMULATIVE ? class_psi(m, B) : class_total(m, B);
  return diag_download(m, out, from, (size_t)count * sizeof(gb25_class_sum));
}

}  // extern "C"
