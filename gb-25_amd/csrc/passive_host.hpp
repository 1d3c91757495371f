// passive_host.hpp -- host side of gb25_tracers_begin / _set / _get / _advance / _stats / _clock / _end (include/gb25.h): passive
// tracers carried beside a run.  Included by gb25_api.hip behind diagnostics_host.hpp, whose shared helpers (diag_*) it uses.
// Kernels: passive_kernels.hpp (k_passive_update) and the one-tracer tendency kernel the closure CATKE uses for e
// (k_tracer_tendencies_single through tendency_instance<SingleKernels> / plan_single), launched with the pointers of a passive tracer.
// Like the diagnostics nothing here writes model memory or a schedule flag; the only memory written is the set's own allocation,
// which the set owns: gb25_tracers_end frees it, gb25_destroy frees the sets still open (passive_release_all).
#pragma once

struct gb25_tracers {
  gb25_model* owner = nullptr;
  int count = 0;
  gb25_tracer_spec spec[PASSIVE_MAX] = {};
  void* base = nullptr;   // ONE allocation: c, G^n, G^- of every tracer, each a parent array of GB25_T
  real *c[PASSIVE_MAX] = {}, *Gn[PASSIVE_MAX] = {}, *Gm[PASSIVE_MAX] = {};
  double time = 0;
  int64_t iteration = 0;
  bool euler_next = true;   // the next advance is an Euler step (the first one; the first after gb25_tracers_set)
};

namespace {

// what a model must be for a set to exist and to advance: each refusal by name, before anything is allocated or launched
gb25_status passive_refusal(gb25_model* m, const char* what) {
  if (gb25_status s = diag_need_device(m, what)) return s;
  if (m->slab) return fail(m, GB25_ERR_STATE, "%s: passive tracers are built for single domains; this model is a rank of a decomposition", what);
  if (m->nu != 0 || m->kappa != 0)
    return fail(m, GB25_ERR_STATE, "%s: passive tracers are built for closure = nothing; gb25_set_vertical_diffusivity is set (nu = %g, kappa = %g)",
                what, m->nu, m->kappa);
  if (m->catke) return fail(m, GB25_ERR_STATE, "%s: passive tracers are built for closure = nothing; closure = CATKEVerticalDiffusivity() is on", what);
  if (m->g.cv.pivot_slaved)
    return fail(m, GB25_ERR_STATE, "%s: passive tracers know the fold without GB25_OPT_FOLD_PIVOT_SLAVED only", what);
  return GB25_OK;
}
gb25_status passive_check_set(gb25_model* m, const gb25_tracers* set, const char* what) {
  if (!set) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: the set is NULL", what);
  if (std::find(m->tracer_sets.begin(), m->tracer_sets.end(), set) == m->tracer_sets.end())
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: this set does not belong to this model (it was begun on another model, or ended)", what);
  return GB25_OK;
}
gb25_status passive_check_index(gb25_model* m, const gb25_tracers* set, int32_t n, const char* what) {
  if (n < 0 || n >= set->count) return fail(m, GB25_ERR_INVALID_ARGUMENT, "%s: tracer n = %d of a set of %d (0-based)", what, (int)n, set->count);
  return GB25_OK;
}
// host <-> one parent array of the shape of GB25_T (copy_field of an array that is no field of the model)
gb25_status passive_copy(gb25_model* m, real* dev, real* host, int include_halos, bool to_device) {
  const Field& F = m->f[GB25_T];
  if (include_halos) {
    if (to_device) HIPCHK(hipMemcpy(dev, host, F.elems() * sizeof(real), hipMemcpyHostToDevice));
    else HIPCHK(hipMemcpy(host, dev, F.elems() * sizeof(real), hipMemcpyDeviceToHost));
    return GB25_OK;
  }
  const Dims d = host_dims(m->layout, GB25_T, false), skip = halo_depth(m->layout, GB25_T);
  hipMemcpy3DParms p = {};
  hipPitchedPtr dv = make_hipPitchedPtr(dev, (size_t)F.nx * sizeof(real), F.nx, F.ny);
  hipPitchedPtr hst = make_hipPitchedPtr(host, (size_t)d.nx * sizeof(real), d.nx, d.ny);
  hipPos dpos = make_hipPos((size_t)skip.nx * sizeof(real), skip.ny, skip.nz), zero = make_hipPos(0, 0, 0);
  p.extent = make_hipExtent((size_t)d.nx * sizeof(real), d.ny, d.nz);
  if (to_device) {
    p.srcPtr = hst; p.srcPos = zero; p.dstPtr = dv; p.dstPos = dpos; p.kind = hipMemcpyHostToDevice;
  } else {
    p.srcPtr = dv; p.srcPos = dpos; p.dstPtr = hst; p.dstPos = zero; p.kind = hipMemcpyDeviceToHost;
  }
  HIPCHK(hipMemcpy3D(&p));
  return GB25_OK;
}
// k_passive_update for tracers [first, first + count) of the set: the update (C1, C2 of the step), or with update = false the mask
// and the halo cells alone
gb25_status passive_launch_update(gb25_model* m, gb25_tracers* set, int first, int count, bool update, real C1, real C2) {
  const Grid& g = m->g;
  PassiveArgs A = {};
  const double dt = m->last_dt;
  for (int q = 0; q < count; q++) {
    const gb25_tracer_spec& sp = set->spec[first + q];
    A.c[q] = set->c[first + q]; A.Gn[q] = set->Gn[first + q]; A.Gm[q] = set->Gm[first + q];
    A.source[q] = (real)(dt * sp.source);
    A.surface[q] = (real)sp.surface_value;
    A.reset[q] = sp.surface_reset != 0;
    A.clip[q] = sp.clip_negative != 0;
  }
  A.dt = (real)dt; A.C1 = C1; A.C2 = C2;
  A.count = count;
  A.fold = is_folded(m) ? 1 : 0;
  const dim3 grid((g.Nx + 63) / 64, (g.Ny + 3) / 4, (unsigned)(g.Nz * count)), block(64, 4);
  if (update) {
    if (m->immersed) hipLaunchKernelGGL((k_passive_update<true, true>), grid, block, 0, m->stream, g, A);
    else hipLaunchKernelGGL((k_passive_update<false, true>), grid, block, 0, m->stream, g, A);
  } else {
    if (m->immersed) hipLaunchKernelGGL((k_passive_update<true, false>), grid, block, 0, m->stream, g, A);
    else hipLaunchKernelGGL((k_passive_update<false, false>), grid, block, 0, m->stream, g, A);
  }
  LAUNCHCHK();
  return GB25_OK;
}
void passive_free(gb25_tracers* set) {
  if (set->base) (void)hipFree(set->base);
  delete set;
}
// gb25_destroy: the sets the user forgot
void passive_release_all(gb25_model* m) {
  for (gb25_tracers* set : m->tracer_sets) passive_free(set);
  m->tracer_sets.clear();
}

}  // namespace

extern "C" {

int32_t gb25_tracer_spec_bytes(void) { return (int32_t)sizeof(gb25_tracer_spec); }

gb25_status gb25_tracers_begin(gb25_model* m, int32_t count, const gb25_tracer_spec* specs, gb25_tracers** out) {
  if (!m || !out) return GB25_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  static_assert(PASSIVE_MAX == GB25_TRACERS_MAX, "gb25.h: GB25_TRACERS_MAX");
  if (count < 1 || count > GB25_TRACERS_MAX)
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_tracers_begin: count = %d must lie in 1 .. %d", (int)count, GB25_TRACERS_MAX);
  if (!specs) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_tracers_begin: specs is NULL");
  for (int q = 0; q < count; q++)
    if (!std::isfinite(specs[q].source) || !std::isfinite(specs[q].surface_value))
      return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_tracers_begin: tracer %d: source = %g and surface_value = %g must be finite", q,
                  specs[q].source, specs[q].surface_value);
  if (gb25_status s = passive_refusal(m, "gb25_tracers_begin")) return s;
  if (m->tracer_order != 5 && m->tracer_order != 7)
    return fail(m, GB25_ERR_STATE, "gb25_tracers_begin: the one-tracer kernel has no variant for tracer advection order %d", m->tracer_order);
  if (gb25_status s = wait_for_model(m)) return s;
  const size_t each = (m->f[GB25_T].elems() * sizeof(real) + 255) & ~(size_t)255, bytes = each * 3 * (size_t)count;
  char of[64];
  snprintf(of, sizeof of, "%d passive tracers", (int)count);
  if (gb25_status s = diag_room_for(m, "gb25_tracers_begin", of, (double)bytes)) return s;
  void* made = nullptr;
  if (gb25_status s = diag_alloc_zeroed(m, "gb25_tracers_begin", of, bytes, &made)) return s;
  gb25_tracers* set = new gb25_tracers();
  set->owner = m;
  set->count = count;
  set->base = made;
  for (int q = 0; q < count; q++) {
    set->spec[q] = specs[q];
    set->c[q] = (real*)((char*)made + each * (3 * (size_t)q));
    set->Gn[q] = (real*)((char*)made + each * (3 * (size_t)q + 1));
    set->Gm[q] = (real*)((char*)made + each * (3 * (size_t)q + 2));
  }
  set->time = m->time;
  set->iteration = m->iteration;
  m->tracer_sets.push_back(set);
  *out = set;
  return GB25_OK;
}

gb25_status gb25_tracers_set(gb25_model* m, gb25_tracers* set, int32_t n, const void* host, int include_halos) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (gb25_status s = passive_check_set(m, set, "gb25_tracers_set")) return s;
  if (gb25_status s = passive_check_index(m, set, n, "gb25_tracers_set")) return s;
  if (!host) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_tracers_set: host is NULL");
  if (gb25_status s = wait_for_model(m)) return s;
  if (gb25_status s = passive_copy(m, set->c[n], static_cast<real*>(const_cast<void*>(host)), include_halos, true)) return s;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    if (gb25_status s = passive_launch_update(m, set, n, 1, false, real(0.), real(0.))) return s;
  }
  HIPCHK(hipStreamSynchronize(m->stream));
  set->euler_next = true;
  return GB25_OK;
}

gb25_status gb25_tracers_get(gb25_model* m, gb25_tracers* set, int32_t n, int32_t which, void* host, int include_halos) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (gb25_status s = passive_check_set(m, set, "gb25_tracers_get")) return s;
  if (gb25_status s = passive_check_index(m, set, n, "gb25_tracers_get")) return s;
  if (which < 0 || which > 2) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_tracers_get: which = %d (0: c, 1: G^n, 2: G^-)", (int)which);
  if (!host) return fail(m, GB25_ERR_INVALID_ARGUMENT, "gb25_tracers_get: host is NULL");
  HIPCHK(hipStreamSynchronize(m->stream));
  // (an advance ends with the exchange of the two pointers: the tendency it made is where the next one looks for G^-)
  real* dev = which == 0 ? set->c[n] : which == 1 ? set->Gm[n] : set->Gn[n];
  return passive_copy(m, dev, static_cast<real*>(host), include_halos, false);
}

gb25_status gb25_tracers_advance(gb25_model* m, gb25_tracers* set) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (gb25_status s = passive_check_set(m, set, "gb25_tracers_advance")) return s;
  if (gb25_status s = passive_refusal(m, "gb25_tracers_advance")) return s;
  if (set->iteration != m->iteration)
    return fail(m, GB25_ERR_STATE, "gb25_tracers_advance: the set is at iteration %lld, the model at iteration %lld: one advance before every "
                "step of the model", (long long)set->iteration, (long long)m->iteration);
  // u, v, w as gb25_get_field would return them, where they live: nothing is pinned or moved (diag_source)
  static const gb25_field ids[3] = {GB25_U, GB25_V, GB25_W};
  const real* src[3];
  for (int q = 0; q < 3; q++)
    if (gb25_status s = diag_source(m, ids[q], &src[q])) return s;
  if (m->route.w_field_stale())   // (only after a composite call that failed half-way)
    if (gb25_status s = materialize_uv(m)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  const Grid& g = m->g;
  const TracerPlan p = plan_single(launch_facts(m));
  // the plain inputs: corrected velocities in memory, the stored w
  const bool curv = g.cv.on;
  SingleKernels::kernel_t kt;
  if (gb25_status s = tendency_instance<SingleKernels>(m, std::array<bool, SingleKernels::n>{m->immersed || curv, curv, m->tracer_order == 7, false}, &kt)) return s;
  const LazyCorr lz{m->corr[0].d, m->corr[1].d, m->wbase, g.sx * g.sy_v};
  const real chi = set->euler_next ? -real(0.5) : (real)m->cfg.chi;
  {
    Timed t(m, GB25_K_DIAGNOSTICS);
    for (int q = 0; q < set->count; q++)
      hipLaunchKernelGGL(kt, dim3(p.nb), dim3(64, 4), 0, m->stream, g, src[0], src[1], src[2], (const real*)set->c[q], set->Gn[q], p.nbx,
                         p.kchunks, p.nb, lz);
    LAUNCHCHK();
    if (gb25_status s = passive_launch_update(m, set, 0, set->count, true, real(1.5) + chi, real(0.5) + chi)) return s;
  }
  HIPCHK(hipStreamSynchronize(m->stream));   // (u, v, w are free for the model's step when the call returns)
  for (int q = 0; q < set->count; q++) std::swap(set->Gn[q], set->Gm[q]);
  set->euler_next = false;
  set->iteration += 1;
  set->time += m->last_dt;
  return GB25_OK;
}

gb25_status gb25_tracers_stats(gb25_model* m, gb25_tracers* set, int32_t n, gb25_field_stats* out) {
  if (!m || !out) return GB25_ERR_INVALID_ARGUMENT;
  if (gb25_status s = passive_check_set(m, set, "gb25_tracers_stats")) return s;
  if (gb25_status s = passive_check_index(m, set, n, "gb25_tracers_stats")) return s;
  DiagBox b;
  if (gb25_status s = diag_scratch(m)) return s;
  if (gb25_status s = diag_box(m, GB25_T, 0, &b)) return s;
  if (gb25_status s = diag_check_box(m, b)) return s;
  if (gb25_status s = wait_for_model(m)) return s;
  return diag_stats_of(m, GB25_T, set->c[n], b, 0, out);
}

gb25_status gb25_tracers_clock(gb25_model* m, gb25_tracers* set, double* time, int64_t* iteration) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (gb25_status s = passive_check_set(m, set, "gb25_tracers_clock")) return s;
  if (time) *time = set->time;
  if (iteration) *iteration = set->iteration;
  return GB25_OK;
}

gb25_status gb25_tracers_end(gb25_model* m, gb25_tracers* set) {
  if (!m) return GB25_ERR_INVALID_ARGUMENT;
  if (gb25_status s = passive_check_set(m, set, "gb25_tracers_end")) return s;
  HIPCHK(hipStreamSynchronize(m->stream));
  m->tracer_sets.erase(std::remove(m->tracer_sets.begin(), m->tracer_sets.end(), set), m->tracer_sets.end());
  passive_free(set);
  return GB25_OK;
}

}  // extern "C"
