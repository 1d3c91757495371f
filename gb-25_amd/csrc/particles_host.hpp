// particles_host.hpp -- host side of gb25_particles_begin / _set / _get / _advance / _sample / _get_info / _end (include/gb25.h);
// included by gb25_api.hip behind diagnostics_host.hpp, whose shared helpers (diag_*) it uses.  Kernels: particle_kernels.hpp; the
// memory: the part_* members of DiagState (diagnostics_state.hpp), freed by its release_particles().  Like the other diagnostics
// nothing here writes model memory or a schedule flag: the only memory written is the particles' own allocation.
#pragma once

namespace {

// the particles' own table: kbot in the parent layout of a (c,f) 2-D field (made anew when the bottom was rebuilt)
gb25_status particles_tables(gb25_model* m) {
  if (m->diag.part_tables_valid) return GB25_OK;
  const int H = m->cfg.halo, sx = m->Nx + 2 * H, sy = m->Ny + 2 * H + 1;
  std::vector<int> kb((size_t)sx * sy);
  for (int j = -H; j < sy - H; j++)
    for (int i = -H; i < sx - H; i++) kb[(size_t)(i + H) + (size_t)sx * (j + H)] = first_wet_level(m, i, j);
  HIPCHK(hipMemcpy(m->diag.part_kbot, kb.data(), kb.size() * sizeof(int), hipMemcpyHostToDevice));
  m->diag.part_tables_valid = true;
  return GB25_OK;
}

gb25_status particles_window(gb25_model* m, const char* what, int64_t first, int64_t count, int64_t limit, const char* of) {
  if (first < 0 || count < 0 || first > limit || count > limit - first)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: window first = %lld, count = %lld of %lld %s", what, (long long)first, (long long)count,
                (long long)limit, of);
  return GB25_OK;
}

}  // namespace

extern "C" {

int32_t gb25_particles_info_bytes(void) { return (int32_t)sizeof(gb25_particles_info); }

gb25_status gb25_particles_begin(gb25_model* m, int64_t capacity) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (capacity <= 0) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_particles_begin: capacity = %lld must be > 0", (long long)capacity);
  if (gb25_status s = diag_need_device(m, "gb25_particles_begin")) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  // one allocation, every part on a multiple of 16 bytes: two copies of the state (3 doubles, 4 ints per particle), the sample
  // array, the per-wave counter slots and their totals, the kbot table
  const int H = m->cfg.halo;
  const size_t table = (size_t)(m->Nx + 2 * H) * (m->Ny + 2 * H + 1);
  const double per_particle = 2.0 * (3 * sizeof(double) + 4 * sizeof(int)) + sizeof(double) + sizeof(unsigned) * GB25_PC_COUNT / 64.0;
  char of[64];
  snprintf(of, sizeof of, "capacity = %lld particles", (long long)capacity);
  const double need = per_particle * (double)capacity + (double)table * sizeof(int) + 4096.0;   // (a double: no capacity overflows it)
  if (gb25_status s = diag_room_for(m, "gb25_particles_begin", of, need)) return s;
  const size_t cap = ((size_t)capacity + 1) & ~(size_t)1;   // (an even number of elements: every array starts on 16 bytes)
  const size_t waves = ((cap + PART_BLOCK - 1) / PART_BLOCK) * (PART_BLOCK / 64);
  size_t bytes = 0;
  auto take = [&](size_t n) { const size_t at = bytes; bytes += (n + 15) & ~(size_t)15; return at; };
  size_t off_d[2][3], off_i[2][4];
  for (int s = 0; s < 2; s++) {
    for (auto& o : off_d[s]) o = take(cap * sizeof(double));
    for (auto& o : off_i[s]) o = take(cap * sizeof(int));
  }
  const size_t off_sample = take(cap * sizeof(double)), off_slots = take(waves * GB25_PC_COUNT * sizeof(unsigned)),
               off_totals = take(GB25_PC_COUNT * sizeof(unsigned long long)), off_kbot = take(table * sizeof(int));
  m->diag.release_particles();   // (a model that already has particles starts over)
  void* made = nullptr;
  if (gb25_status s = diag_alloc_zeroed(m, "gb25_particles_begin", of, bytes, &made)) return s;
  char* base = (char*)made;
  m->diag.part_base = base;
  for (int s = 0; s < 2; s++) {
    PartState& P = m->diag.part_state[s];
    P.a = (double*)(base + off_d[s][0]); P.b = (double*)(base + off_d[s][1]); P.c = (double*)(base + off_d[s][2]);
    P.i = (int*)(base + off_i[s][0]); P.j = (int*)(base + off_i[s][1]); P.k = (int*)(base + off_i[s][2]);
    P.status = (int*)(base + off_i[s][3]);
  }
  m->diag.part_sample = (double*)(base + off_sample);
  m->diag.part_slots = (unsigned*)(base + off_slots);
  m->diag.part_totals = (unsigned long long*)(base + off_totals);
  m->diag.part_kbot = (int*)(base + off_kbot);
  m->diag.part_info.capacity = capacity;
  m->diag.part_on = true;
  return GB25_OK;
}

gb25_status gb25_particles_set(gb25_model* m, int64_t first, int64_t count, const int32_t* i, const int32_t* j, const int32_t* k,
                               const double* a, const double* b, const double* c) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->diag.part_on) return fail(m, GB25_ERR_STATE, "gb25_particles_set: this model has no particles (call gb25_particles_begin first)");
  gb25_particles_info& I = m->diag.part_info;
  if (gb25_status s = particles_window(m, "gb25_particles_set", first, 0, I.count, "particles so far (first may append, not leave a gap)")) return s;
  if (gb25_status s = particles_window(m, "gb25_particles_set", first, count, I.capacity, "(the capacity)")) return s;
  if (count > 0 && (!i || !j || !k || !a || !b || !c)) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_particles_set: an array is NULL with count = %lld", (long long)count);
  const int Nz = m->cfg.Nz;
  for (int64_t n = 0; n < count; n++) {
    if (i[n] < 0 || i[n] >= m->Nx || j[n] < 0 || j[n] >= m->Ny || k[n] < 0 || k[n] >= Nz)
      return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_particles_set: particle %lld: cell i, j, k = %d, %d, %d is outside the interior %d x %d x %d",
                  (long long)(first + n), (int)i[n], (int)j[n], (int)k[n], m->Nx, m->Ny, Nz);
    if (!(a[n] >= 0.0 && a[n] < 1.0 && b[n] >= 0.0 && b[n] < 1.0 && c[n] >= 0.0 && c[n] < 1.0))
      return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_particles_set: particle %lld: fraction a, b, c = %.17g, %.17g, %.17g must lie in [0, 1)",
                  (long long)(first + n), a[n], b[n], c[n]);
    if (k[n] < first_wet_level(m, i[n], j[n]))
      return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_particles_set: particle %lld: cell i, j, k = %d, %d, %d is dry (the column's first wet level is %d)",
                  (long long)(first + n), (int)i[n], (int)j[n], (int)k[n], first_wet_level(m, i[n], j[n]));
  }
  if (count > 0) {
    const PartState& P = m->diag.part_state[m->diag.part_cur];
    const size_t ni = (size_t)count * sizeof(int), nd = (size_t)count * sizeof(double);
    HIPCHK(hipMemcpyAsync(P.i + first, i, ni, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(P.j + first, j, ni, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(P.k + first, k, ni, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(P.a + first, a, nd, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(P.b + first, b, nd, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemcpyAsync(P.c + first, c, nd, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipMemsetAsync(P.status + first, 0, ni, m->stream));   // (GB25_PARTICLE_ACTIVE)
    HIPCHK(hipStreamSynchronize(m->stream));   // (the host arrays are borrowed for the duration of the call)
  }
  I.count = first + count;
  return GB25_OK;
}

gb25_status gb25_particles_get(gb25_model* m, int64_t first, int64_t count, int32_t* i, int32_t* j, int32_t* k, double* a, double* b,
                               double* c, int32_t* status) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->diag.part_on) return fail(m, GB25_ERR_STATE, "gb25_particles_get: this model has no particles (call gb25_particles_begin first)");
  if (gb25_status s = particles_window(m, "gb25_particles_get", first, count, m->diag.part_info.count, "particles")) return s;
  if (count == 0) return GB25_OK;
  const PartState& P = m->diag.part_state[m->diag.part_cur];
  const size_t ni = (size_t)count * sizeof(int), nd = (size_t)count * sizeof(double);
  if (i) HIPCHK(hipMemcpyAsync(i, P.i + first, ni, hipMemcpyDeviceToHost, m->stream));
  if (j) HIPCHK(hipMemcpyAsync(j, P.j + first, ni, hipMemcpyDeviceToHost, m->stream));
  if (k) HIPCHK(hipMemcpyAsync(k, P.k + first, ni, hipMemcpyDeviceToHost, m->stream));
  if (a) HIPCHK(hipMemcpyAsync(a, P.a + first, nd, hipMemcpyDeviceToHost, m->stream));
  if (b) HIPCHK(hipMemcpyAsync(b, P.b + first, nd, hipMemcpyDeviceToHost, m->stream));
  if (c) HIPCHK(hipMemcpyAsync(c, P.c + first, nd, hipMemcpyDeviceToHost, m->stream));
  if (status) HIPCHK(hipMemcpyAsync(status, P.status + first, ni, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(hipStreamSynchronize(m->stream));
  return GB25_OK;
}

gb25_status gb25_particles_advance(gb25_model* m, double dt, int32_t substeps) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->diag.part_on) return fail(m, GB25_ERR_STATE, "gb25_particles_advance: this model has no particles (call gb25_particles_begin first)");
  if (!(std::isfinite(dt) && dt > 0.0)) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_particles_advance: dt must be finite and > 0, got %g", dt);
  if (substeps <= 0) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_particles_advance: substeps must be > 0, got %d", (int)substeps);
  static const gb25_field ids[3] = {GB25_U, GB25_V, GB25_W};
  const real* src[3];
  for (int q = 0; q < 3; q++)
    if (gb25_status s = diag_source(m, ids[q], &src[q])) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = particles_tables(m)) return s;
  gb25_particles_info& I = m->diag.part_info;
  unsigned long long totals[GB25_PC_COUNT] = {};
  if (I.count > 0) {
    const Grid& g = m->g;
    PartArgs A;
    A.in = m->diag.part_state[m->diag.part_cur];
    A.out = m->diag.part_state[m->diag.part_cur ^ 1];
    A.u = src[0]; A.v = src[1]; A.w = src[2];
    A.dxu = g.cv.on ? g.cv.dxfc : g.dxc;
    A.dyv = g.cv.on ? g.cv.dycf : nullptr;
    A.dzc = g.dzc;
    A.kbot = m->diag.part_kbot;
    A.slots = m->diag.part_slots;
    A.dy = (double)g.dy;
    A.h = dt / (double)substeps;
    A.n = I.count;
    A.substeps = substeps;
    A.Nx = g.Nx; A.Ny = g.Ny; A.Nz = g.Nz; A.H = g.H; A.sx = g.sx; A.pl_c = g.pl_c; A.pl_v = g.pl_v;
    A.x_periodic = g.x_periodic;
    A.fold = is_folded(m) ? 1 : 0;
    A.j_south = g.jws;
    A.j_north = A.fold ? g.Ny : g.jwn;
    const unsigned blocks = (unsigned)((I.count + PART_BLOCK - 1) / PART_BLOCK);
    {
      Timed t(m, GB25_K_DIAGNOSTICS);
      if (g.cv.on) hipLaunchKernelGGL(k_particles_advance<true>, dim3(blocks), dim3(PART_BLOCK), 0, m->stream, A);
      else hipLaunchKernelGGL(k_particles_advance<false>, dim3(blocks), dim3(PART_BLOCK), 0, m->stream, A);
      LAUNCHCHK();
      hipLaunchKernelGGL(k_particles_fold, dim3(1), dim3(PART_BLOCK), 0, m->stream, (const unsigned*)m->diag.part_slots,
                         (long long)blocks * (PART_BLOCK / 64), m->diag.part_totals);
      LAUNCHCHK();
    }
    if (gb25_status s = diag_download(m, totals, m->diag.part_totals, sizeof totals)) return s;   // (the sources are free for the next step when the call returns)
  }
  if (totals[GB25_PC_TOO_FAR]) {   // (the copy that was read stays the state: no particle has moved)
    for (int q = 0; q < GB25_PC_COUNT; q++) I.last[q] = 0;
    I.last[GB25_PC_TOO_FAR] = (int64_t)totals[GB25_PC_TOO_FAR];
    I.total[GB25_PC_TOO_FAR] += (int64_t)totals[GB25_PC_TOO_FAR];
    return fail(m, GB25_ERR_STATE, "gb25_particles_advance: %llu particle%s would leave the rank by more than one cell per call: more substeps "
                "or a shorter dt (dt = %g, substeps = %d)", totals[GB25_PC_TOO_FAR], totals[GB25_PC_TOO_FAR] == 1 ? "" : "s", dt, (int)substeps);
  }
  if (I.count > 0) m->diag.part_cur ^= 1;
  for (int q = 0; q < GB25_PC_COUNT; q++) {
    I.last[q] = (int64_t)totals[q];
    I.total[q] += (int64_t)totals[q];
  }
  I.calls++;
  I.substeps += substeps;
  I.time_advanced = I.time_advanced + dt;
  return GB25_OK;
}

gb25_status gb25_particles_sample(gb25_model* m, gb25_field f, double* out, int64_t count) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (!m->diag.part_on) return fail(m, GB25_ERR_STATE, "gb25_particles_sample: this model has no particles (call gb25_particles_begin first)");
  if (f < 0 || f >= GB25_FIELD_COUNT || moments_loc(f) != LOC_CCC)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_particles_sample: field %d is not a (c,c,c) field (T, S, e, pHY and their tendencies are)", (int)f);
  if (count != m->diag.part_info.count)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_particles_sample: count is %lld, the model has %lld particles", (long long)count,
                (long long)m->diag.part_info.count);
  if (count > 0 && !out) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_particles_sample: out is NULL");
  const real* src = nullptr;
  if (gb25_status s = diag_source(m, f, &src)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  if (count == 0) return GB25_OK;
  const Grid& g = m->g;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    hipLaunchKernelGGL(k_particles_sample, dim3((unsigned)((count + PART_BLOCK - 1) / PART_BLOCK)), dim3(PART_BLOCK), 0, m->stream,
                       m->diag.part_state[m->diag.part_cur], src, m->diag.part_sample, (long long)count, g.Nx, g.Ny, g.Nz, g.H, g.sx, g.pl_c);
    LAUNCHCHK();
  }
  return diag_download(m, out, m->diag.part_sample, (size_t)count * sizeof(double));
}

gb25_status gb25_particles_get_info(const gb25_model* m, gb25_particles_info* info) {
  if (!m || !info) return GB25_ERR_INVALID_ARGUMENT;
  *info = m->diag.part_info;   // (all zero while the model has no particles)
  return GB25_OK;
}

gb25_status gb25_particles_end(gb25_model* m) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (m->diag.part_on) HIPCHK(hipStreamSynchronize(m->stream));
  m->diag.release_particles();
  return GB25_OK;
}

}  // extern "C"
