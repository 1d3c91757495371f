// slab_step.hpp -- the time step of an x-slab decomposition, inside the library.
//
// Replaces what the reference gets from `Oceananigans.Distributed(arch; partition=Partition(Rx, Ry, 1))` + XLA's SPMD
// partitioner (GB-25 sharding/sharded_baroclinic_instability_simulation_run.jl:65-72,145-164): there `loop!(model,
// Ninner)` is ONE executable whose halo copies XLA turned into collective-permutes (ncclSend/Recv kernels); here
// gb25_loop on a slab is one call that sequences the stages of the step, the pack / unpack kernels and the
// point-to-point exchanges on two HIP streams.  Three transports move the packed columns:
//   * RCCL  (product, one process per GPU): ncclGroupStart; ncclSend/ncclRecv to west and east; ncclGroupEnd on the
//            stream the exchange belongs to.  librccl is loaded at run time (dlopen), so the library itself has no
//            link-time dependency and loads on a machine without RCCL (where only single-domain models are built).
//   * local (several slabs of one decomposition in ONE process, same device): device-to-device copies.  This is what the
//            decomposition-invariance tests run at full size on a one-GPU box.
//   * host callback (rehearsal of the multi-process path where RCCL cannot run, e.g. two ranks on one device): the host
//            moves the buffers; synchronous.
// The sequencing itself (`sequence_time_step`) is written against an abstract StepOps so that a dry run can record the
// order of operations without a GPU (gb25_debug_sequence; tests/test_distributed_cpu.py).
//
//   (stages, groups, buffer sets, streams and event slots by name and number: slab_protocol.hpp; the table of groups: DESIGN.md)
//   Update (stage 0)  AB2 update of u,v,T,S (adoption of the look-aheads), y/z layers of the 3-D bundle; pressure of the own
//             columns starts on the slab's side stream                                            (main stream)
//   Bundle (group 0)  H columns of u,v,T,S  -> x halos        packed + sent on the COMM stream, in flight during OwnColumns
//   OwnColumns (2)    barotropic corrector on the own columns, their y/z layers, w on the own columns, momentum tendencies of
//             the INTERIOR tile columns                                              (main stream)
//   HaloColumns (3)   [wait for Bundle] corrector in the halo columns, w and p' strips, momentum tendencies of the edge tile
//             columns                                                                                (main stream)
//   Tracers (4)       tracer tendencies                                                             (main stream)
//     beside Tracers, on the COMM stream, the sub-cycle of the NEXT step (its G.U, G.V exist since HaloColumns):
//   BaroWideAhead (3) W = Ns+1+H columns of eta,U,V and of the next G.U,G.V -> wide barotropic halos
//   SubcycleAhead (5) Ns split-explicit substeps on the widened slab into the partner buffers of eta,U,V, filtered state; the slab
//             is wide enough that the x HALO columns of the new eta,U,V come out valid too: nothing is exchanged after it
//   The next Update adopts them.  When a look-ahead is not valid (first step, changed dt, host writes) the same work
//   runs inside the step instead: BaroWide (1), Subcycle (1), on the critical path.  (BaroHalo, 2 -- H columns of eta,U,V --
//   remains for the initial state.)
//   Folded (tripolar) grid: the work arrays of the sub-cycle are also TALL -- Wy rows beyond the pivot row, the images of the
//   partner rank's rows south of it -- so between Subcycle / SubcycleAhead (which then only copy the interiors) and the substeps
//   (SubcycleSubsteps 16 / SubcycleAheadSubsteps 56) one more exchange, FoldTall (8), carries those rows to the partner: ONE partner
//   exchange per step for the sub-cycle, none inside it.  FoldBundle (6) is the partner exchange of the 3-D bundle's rows (and of
//   eta, U, V): HaloColumnsToLayers (30) before it, HaloColumnsRest (31) after.
//   2-D decomposition (Partition(Rx, Ry, 1), cfg.ranks_y > 1): every exchange in x is followed by the exchange of whole rows with
//   the southern / northern neighbour, which carry the x halo columns just received (the corners): BaroWideRows (11) /
//   BaroWideRowsAhead (13) after BaroWide / BaroWideAhead and the interior copy (the work arrays are widened in y as in x),
//   BundleRows (10) after Bundle and the corrector of the own rows' x halo columns (HaloRowsCorrector, 32: the rows arrive
//   corrected), BaroHaloRows (12) after BaroHalo.  The fold partner is the mirrored rank of the top row.  No interior / edge split
//   of the tendencies and no early pressure on such a rank.
//   closure = CATKE: e and J^b travel once more per update_state!, after the step of e (CatkeColumns 20, CatkeRows 21, CatkeFold
//   22), then CatkeFinish (41).
#pragma once
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <array>
#include <string>
#include <vector>

#include "slab_protocol.hpp"

// (included by gb25_api.hip after the model and its phase implementations)

namespace {

// ---- x-slab exchange pieces: the columns of a Mover::Columns group (what each group is: slab_protocol.hpp) --------------------
struct Piece {
  real* src;      // array that is packed from (canonical layout)
  real* dst;      // array that is unpacked into
  int src_sx, src_xo, dst_sx, dst_xo;
  long rows;
};
void group_pieces(gb25_model* m, Group group, std::vector<Piece>& out, int* ncols) {
  const int H = m->cfg.halo, sx = m->Nx + 2 * H;
  auto whole = [&](real* p, long rows) { out.push_back({p, p, sx, H, sx, H, rows}); };   // H columns, unpacked where they came from
  *ncols = H;
  switch (group) {
    case Group::CatkeColumns:
      // the TKE tracer after its step inside compute_diffusivities!, and the filtered J^b (kappa of the first halo column is
      // COMPUTED from them)
      if (!m->catke) return;
      for (int id : {GB25_E, GB25_JB}) whole(m->f[id].d, (long)m->f[id].ny * m->f[id].nz);
      return;
    case Group::Bundle:
      for (int id : {GB25_U, GB25_V, GB25_T, GB25_S}) whole(m->f[id].d, (long)m->f[id].ny * m->f[id].nz);
      // the column integrals of u, v (the corrector's): the receiver corrects its halo columns cell by cell with them
      for (int q = 0; q < 2; q++) whole(m->colsum[q].d, (long)m->colsum[q].ny);
      // ... and their sums over the momentum kernel's chunks of levels (w on the fly: the chunk bases of w next to the x halos)
      if (slab_wfly_ok(m)) {
        const int kch = mom_kchunks(m);
        const long plane2 = (long)m->g.sx * m->g.sy_v;
        for (int q = 2; q < 4; q++) whole(m->uv_partials + (long)q * kch * plane2, (long)kch * m->g.sy_v);
      }
      return;
    case Group::BaroHalo:
      for (int q = 0; q < 3; q++) whole(m->f[GB25_ETA + q].d, (long)m->f[GB25_ETA + q].ny * m->f[GB25_ETA + q].nz);
      return;
    case Group::BaroWide:
    case Group::BaroWideAhead: {
      *ncols = m->W;
      const int wsx = m->Nx + 2 * m->W;
      const size_t up = (size_t)m->Wys * wsx;   // (2-D decomposition: the work arrays start Wys rows below the canonical ones)
      for (int q = 0; q < 3; q++) {
        Field& F = m->f[GB25_ETA + q];
        out.push_back({F.d, m->wide[0][q].d + up, sx, H, wsx, m->W, (long)F.ny});
      }
      for (int q = 0; q < 2; q++) {
        Field& F = group == Group::BaroWide ? m->f[GB25_GN_BT_U + q] : m->ahead_G[q];
        out.push_back({F.d, m->wideG[q].d + up, sx, H, wsx, m->W, (long)F.ny});
      }
      return;
    }
    default: return;   // (no columns: the unused groups and those of the other movers)
  }
}
int64_t halo_buffer_elems(gb25_model* m, Group group) {
  std::vector<Piece> ps;
  int nc = 0;
  group_pieces(m, group, ps, &nc);
  int64_t t = 0;
  for (auto& p : ps) t += p.rows * nc;
  return t > 0 ? t : 1;
}
// Both sides of a group in ONE launch (a group is up to ten small strips); buf[side] = that side's contiguous buffer.
gb25_status pack_unpack(gb25_model* m, Group group, real* const buf[2], bool pack) {
  std::vector<Piece> ps;
  int nc = 0;
  group_pieces(m, group, ps, &nc);
  ColumnPieces P{};
  P.ncols = nc;
  long max_n = 0;
  for (int side = 0; side < 2; side++) {
    size_t off = 0;
    for (auto& p : ps) {
      const int f = P.n++;
      P.rows[f] = p.rows;
      P.buf[f] = buf[side] + off;
      if (pack) {   // west side: interior columns [0, nc); east side: [Nx-nc, Nx)
        P.arr[f] = p.src; P.sx[f] = p.src_sx; P.i0[f] = p.src_xo + (side == 0 ? 0 : m->Nx - nc);
      } else {      // west halo: columns [-nc, 0); east halo: [Nx, Nx+nc)
        P.arr[f] = p.dst; P.sx[f] = p.dst_sx; P.i0[f] = p.dst_xo + (side == 0 ? -nc : m->Nx);
      }
      off += (size_t)p.rows * nc;
      max_n = std::max(max_n, p.rows * nc);
    }
  }
  dim3 gr((unsigned)((max_n + 255) / 256), (unsigned)P.n);
  if (pack) hipLaunchKernelGGL(k_move_columns<true>, gr, dim3(256), 0, m->stream, P);
  else hipLaunchKernelGGL(k_move_columns<false>, gr, dim3(256), 0, m->stream, P);
  LAUNCHCHK();
  return GB25_OK;
}

// ---- y halos of a 2-D (x, y) decomposition: whole rows (every parent column) to the southern / northern neighbour ------------
// BundleRows travels after Bundle and the barotropic corrector of the own rows (x halo columns included: the corners), so that the
// rows arrive corrected, as the rows beyond a fold do (FoldBundle); BaroWideRows after BaroWide and the interior copy.
// side 0: southern edge / halo, side 1: northern.  Rows [0, n) / [Ny - n, Ny) are packed, [-n, 0) / [Ny, Ny + n) unpacked.
inline bool y_neighbour(const gb25_model* m, int side) { return side == 0 ? m->ys_open : m->yn_open; }
void row_pieces(gb25_model* m, Group group, int side, bool pack, real* buf, RowPieces& P) {
  const Grid& g = m->g;
  const int H = g.H;
  P = RowPieces{};
  size_t off = 0;
  auto add = [&](real* arr, int sx, int yoff, long pl, int k0, int nz, int nrows) {
    const int f = P.n++;
    const int j = pack ? (side == 0 ? 0 : g.Ny - nrows) : (side == 0 ? -nrows : g.Ny);
    P.arr[f] = arr; P.buf[f] = buf + off; P.sx[f] = sx; P.r0[f] = j + yoff; P.pl[f] = pl; P.k0[f] = k0; P.nz[f] = nz;
    P.nrows = nrows;
    off += (size_t)nz * nrows * sx;
  };
  switch (group) {
    case Group::CatkeRows:   // (the TKE tracer after its step, and J^b for kappa in the first halo row)
      if (m->catke) {
        Field& F = m->f[GB25_E];
        add(F.d, g.sx, H, (long)g.sx * F.ny, H, g.Nz, H);
        add(m->f[GB25_JB].d, g.sx, H, 0, 0, 1, H);
      }
      return;
    case Group::BundleRows:
      for (int id : {GB25_U, GB25_V, GB25_T, GB25_S}) {
        Field& F = m->f[id];
        add(F.d, g.sx, H, (long)g.sx * F.ny, H, g.Nz, H);
      }
      if (slab_lazy_ok(m)) {
        // the corrector inside its consumers: the column integrals of u, v of the rows (the receiver's du, dv there) and, for w on
        // the fly, their sums over the chunks of levels
        for (int q = 0; q < 2; q++) add(m->colsum[q].d, g.sx, H, 0, 0, 1, H);
        if (slab_wfly_ok(m)) {
          const int kch = mom_kchunks(m);
          const long plane2 = (long)g.sx * g.sy_v;
          for (int q = 2; q < 4; q++) add(m->uv_partials + (long)q * kch * plane2, g.sx, H, plane2, 0, kch, H);
        }
      }
      return;
    case Group::BaroWideRows:
    case Group::BaroWideRowsAhead: {
      const int wsx = g.Nx + 2 * m->W;
      for (int q = 0; q < 3; q++) add(m->wide[0][q].d, wsx, H + m->Wys, 0, 0, 1, m->W);
      for (int q = 0; q < 2; q++) add(m->wideG[q].d, wsx, H + m->Wys, 0, 0, 1, m->W);
      return;
    }
    case Group::BaroHaloRows:
      for (int q = 0; q < 3; q++) add(m->f[GB25_ETA + q].d, g.sx, H, 0, 0, 1, H);
      return;
    default: return;   // (no rows: the unused groups and those of the other movers)
  }
}
int64_t row_buffer_elems(gb25_model* m, Group group) {
  if (m->Ry < 2) return 1;
  RowPieces P;
  row_pieces(m, group, 0, true, nullptr, P);
  int64_t t = 0;
  for (int f = 0; f < P.n; f++) t += (int64_t)P.nz[f] * P.nrows * P.sx[f];
  return t > 0 ? t : 1;
}
gb25_status move_rows(gb25_model* m, Group group, real* const buf[2], bool pack) {
  for (int side = 0; side < 2; side++) {
    if (!y_neighbour(m, side)) continue;
    RowPieces P;
    row_pieces(m, group, side, pack, buf[side], P);
    if (P.n == 0) continue;
    int nzmax = 1, sxmax = 0;
    for (int f = 0; f < P.n; f++) { nzmax = std::max(nzmax, P.nz[f]); sxmax = std::max(sxmax, P.sx[f]); }
    const dim3 gr((unsigned)(((long)sxmax * P.nrows + 255) / 256), nzmax, P.n);
    if (pack) hipLaunchKernelGGL(k_move_rows<true>, gr, dim3(256), 0, m->stream, P);
    else hipLaunchKernelGGL(k_move_rows<false>, gr, dim3(256), 0, m->stream, P);
  }
  LAUNCHCHK();
  return GB25_OK;
}

// ---- zipper fold of a decomposed tripolar grid: the partner rank P-1-r holds the cells beyond this slab's fold line -----
// FoldBundle, CatkeFold: H rows south of the pivot row (all parent columns, interior levels); FoldTall: TallRows, kernels.hpp
FoldFields fold_fields(gb25_model* m, bool closure = false) {   // closure: CatkeFold -- e and J^b after the e step
  FoldFields F{};
  const Grid& g = m->g;
  long off = 0;
  auto add = [&](real* p, int is_v, int xf, int neg, int nz) {
    const int f = F.n++;
    F.p[f] = p; F.is_v[f] = is_v; F.xf[f] = xf; F.neg[f] = neg; F.nz[f] = nz; F.off[f] = off;
    off += (long)nz * g.H * g.sx;
  };
  if (closure) {
    if (m->catke) {
      add(m->f[GB25_E].d, 0, 0, 0, g.Nz);
      add(m->f[GB25_JB].d, 0, 0, 0, 1);
    }
    return F;
  }
  add(m->f[GB25_U].d, 0, 1, 1, g.Nz);
  add(m->f[GB25_V].d, 1, 0, 1, g.Nz);
  add(m->f[GB25_T].d, 0, 0, 0, g.Nz);
  add(m->f[GB25_S].d, 0, 0, 0, g.Nz);
  add(m->f[GB25_ETA].d, 0, 0, 0, 1);
  add(m->f[GB25_BT_U].d, 0, 1, 1, 1);
  add(m->f[GB25_BT_V].d, 1, 0, 1, 1);
  return F;
}
int fold_levels(const FoldFields& F, bool with_layers) {   // blockIdx.z extent of k_fold_pack / k_fold_unpack
  int t = 0;
  for (int f = 0; f < F.n; f++) t += F.nz[f] == 1 ? 1 : F.nz[f] + (with_layers ? 2 : 0);
  return t;
}
int64_t fold_buffer_elems(gb25_model* m, bool closure) {
  const Grid& g = m->g;
  return std::max<int64_t>(1, (int64_t)g.H * g.sx * fold_levels(fold_fields(m, closure), false));
}
// Elements per side of buffer set b on this slab: what the set's group packs (the others of the set carry pieces of the same sizes)
int64_t set_elems(gb25_model* m, BufferSet b) {
  const GroupInfo& info = set_info(b);
  switch (info.mover) {
    case Mover::Columns: return halo_buffer_elems(m, info.group);
    case Mover::Rows: return row_buffer_elems(m, info.group);
    case Mover::FoldRows: return m->g.cv.north_fold ? fold_buffer_elems(m, info.closure) : 1;
    case Mover::TallRows: return m->g.cv.north_fold ? tall_buffer_elems(m) : 1;
  }
  return 1;
}
gb25_status fold_pack(gb25_model* m, real* buf, bool closure = false) {
  const Grid& g = m->g;
  FoldFields F = fold_fields(m, closure);
  if (F.n == 0) return GB25_OK;
  hipLaunchKernelGGL(k_fold_pack, dim3((g.sx + 255) / 256, g.H, fold_levels(F, false)), dim3(256), 0, m->stream, g, F, buf);
  LAUNCHCHK();
  return GB25_OK;
}
gb25_status fold_unpack(gb25_model* m, const real* buf, bool closure = false) {
  const Grid& g = m->g;
  FoldFields F = fold_fields(m, closure);
  if (F.n == 0) return GB25_OK;
  hipLaunchKernelGGL(k_fold_unpack, dim3((g.sx + 255) / 256, g.H, fold_levels(F, true)), dim3(256), 0, m->stream, g, F, buf,
                     m->rx * m->Nx, m->cfg.Nx);
  LAUNCHCHK();
  return GB25_OK;
}

// the pressure strips next to the x halos on the exchange stream, right behind the unpacked bundle (plain x slabs, no closure
// whose fields and fills sit in between)
inline bool strips_on_comm(const gb25_model* m) {
  return m->early_strips && m->two_streams && m->pressure_bits == 64 && m->Ry == 1 && !m->catke;
}

// closure = CATKE on a rank of a decomposition.  compute_diffusivities! steps e on the own columns (time_step_catke_equation!)
// and filters J^b there; the diffusivities of the first halo column / row and the advection of e then need the NEW e and J^b of
// the neighbours: one more exchange per update_state! (CatkeColumns: x columns, CatkeRows: rows of a 2-D decomposition, CatkeFold: the rows
// beyond a zipper fold), between these two halves.
gb25_status catke_step_local(gb25_model* m) {
  gb25_status s;
  if ((s = catke_tke_step_impl(m))) return s;
  return fill_halos_impl(m, FillRequest::e(Columns::Own));   // y/z layers of the new e on the own columns: the packed columns travel complete
}
gb25_status catke_finish_local(gb25_model* m) {
  gb25_status s;
  if ((s = fill_halos_impl(m, FillRequest::e(Columns::Extended)))) return s;   // y/z layers of e over the extended range (the halo rows' bottom / top layers)
  if ((s = catke_diffusivities_finish_impl(m))) return s;
  return catke_tendency_impl(m);
}

// ---- the stages of one slab's time step (see the header of this file): one function per family, slab_stage picks the sub-case ----
// own columns' pressure early, on the side stream.  (A folded slab too: the pressure of a cell and its differences to the west
// and south never look north -- what arrives last, the rows beyond the fold, is no input of theirs; the pressure of halo cells
// is not stored inside a composite step.)
// (a rank of a 2-D decomposition computes its pressure in one pass once all halos are in: the early pass plus a one-row strip
// for the y difference of row 0 measured slower on the one-rank proxy, 0.566 against 0.537 ms -- profiles/r03_tuning_log.md)
inline bool pressure_early(const gb25_model* m) { return m->two_streams && m->pressure_bits == 64 && m->Ry == 1; }
// Forks to the slab's side stream: the pressure of `box` there, beside what the calling stream goes on with; ev_join marks its end.
gb25_status pressure_on_side_stream(gb25_model* m, PressureBox box) {
  HIPCHK(hipEventRecord(m->ev_fork, m->stream));
  HIPCHK(hipStreamWaitEvent(m->side_stream, m->ev_fork, 0));
  {
    OnStream on(m, m->side_stream);
    if (gb25_status s = compute_p_impl(m, box, true)) return s;
  }
  HIPCHK(hipEventRecord(m->ev_join, m->side_stream));
  return GB25_OK;
}

// Update: AB2 update of u,v,T,S + barotropic forcing, then the y/z boundary layers of the 3-D bundle so that its packed x columns
// (Bundle) can travel WHILE the own columns are corrected
gb25_status stage_update(gb25_model* m, int euler) {
  gb25_status s;
  const double dt = m->last_dt;
  const real chi = euler ? -real(0.5) : (real)m->cfg.chi;
  const bool uv_adopted = m->valid.velocities_adoptable((real)dt, chi);
  m->baro_adopted = uv_adopted && m->valid.ahead_baro_valid;
  m->valid.void_subcycle_lookahead();
  // The corrector inside its consumers (as on a single domain, time_step_impl): when everything this step needs was made
  // ahead of time, no sweep over u and v -- 2-D kernels leave du, dv (own columns in OwnColumns, halo columns in HaloColumns from
  // the column integrals the bundle carries) and the kernels that read u, v add them.  Memory holds the uncorrected velocities
  // until the composite call returns (gb25_loop).
  // ... and with it w on the fly: no k_compute_w launch, the tendency kernels carry w up their chunks of levels from 2-D bases
  const Corrector corrector = choose_corrector(m, false, uv_adopted, m->baro_adopted);
  if (corrector == Corrector::Sweep && (s = materialize_uv(m))) return s;   // (the sweeps below expect corrected velocities)
  m->route.begin(corrector, route_carries_w(m, corrector));
  if ((s = ab2_local_impl(m, (real)dt, chi))) return s;
  if (m->baro_adopted) {
    // the sub-cycle of this step, its wide-halo exchange and the exchange of the new eta, U, V columns all ran beside the last
    // tracer kernel (SubcycleAhead): adopt the results, Subcycle and BaroWide are skipped
    adopt_subcycle(m);
    m->time += dt;
    m->iteration += 1;
  }
  if ((s = fill_halos_impl(m, FillRequest::uvts(Columns::Own)))) return s;
  // T, S of the slab's own columns are final from here on: their pressure (fp64-bound) runs on the side stream beside the
  // exchanges and the sub-cycle; the strips next to the x halos follow in HaloColumns.  The first x difference of this pass reads
  // a stale halo column and is redone by the west strip.
  return pressure_early(m) ? pressure_on_side_stream(m, PressureBox::own_columns(launch_facts(m))) : GB25_OK;
}

// Subcycle: BaroWide has been unpacked into the wide halos: copy the interiors, sub-cycle, publish.
// ahead: the same for the NEXT step: BaroWideAhead has been unpacked, G.U, G.V come from the momentum look-ahead, the results go
//        to the partner buffers of eta, U, V and of the filtered state.
// Fold / 2-D decomposition: the first call ends after the interior copy (more rows of the work arrays travel next: FoldTall,
// BaroWideRows), a second one with substeps_only does the rest.
gb25_status stage_subcycle(gb25_model* m, bool ahead, bool substeps_only) {
  const Grid& g = m->g;
  gb25_status s;
  const double dt = m->last_dt;
  if (ahead && !m->valid.ahead_uv_valid) return fail(m, GB25_ERR_STATE, "stage 5 without a velocity look-ahead");
  if (!ahead && m->baro_adopted) return fail(m, GB25_ERR_STATE, "stage 1 after stage 0 adopted the sub-cycle");
  std::vector<Piece> ps;
  int nc = 0;
  group_pieces(m, ahead ? Group::BaroWideAhead : Group::BaroWide, ps, &nc);
  const bool two_halves = g.cv.north_fold || m->Ry > 1;
  ColumnCopies C;
  if (!substeps_only) {
    for (auto& p : ps) C.add(p.dst, p.dst_sx, p.dst_xo, p.src, p.src_sx, p.src_xo, (int)p.rows);
    // (a plain slab hands the copy to the sub-cycle: its one-launch kernel reads the own columns where they are)
    if (two_halves) C.launch(m, C.rmax);
  }
  LAUNCHCHK();
  if (two_halves && !substeps_only) return GB25_OK;
  const SubcycleDone done = barotropic_impl(m, ahead ? m->valid.ahead_uv_dt : (real)dt, ahead, two_halves ? nullptr : &C);
  if (done.status) return done.status;
  if (ahead) {
    Halo2 h2{};
    for (int q = 0; q < 3; q++) { h2.p[q] = m->ahead_eta[q].d; h2.is_v[q] = q == 2; }
    h2.n = 3;
    // y layer, x halo columns included: the widened sub-cycle computed those like the neighbour did (no BaroHaloAhead)
    if (!done.layers_written && (s = fill_halos_impl(m, FillRequest::flat_extended(Fields2::Given), h2))) return s;
    m->valid.record_subcycle_lookahead();
    return GB25_OK;
  }
  m->time += dt;
  m->iteration += 1;
  // y layer of the new eta, U, V, x halo columns included (computed by the widened sub-cycle: no BaroHalo)
  return done.layers_written ? GB25_OK : fill_halos_impl(m, FillRequest::flat_extended());
}

// OwnColumns: everything that needs nothing from the neighbours runs while the exchanges are in flight: the barotropic corrector
// on the slab's own columns and, when the tendency kernels are split (a12), the y/z layers and w of the own columns and the
// momentum tendencies of the interior tile columns.
// head_only (LazyHead): the head of a lazy step -- du, dv and the chunk bases of w -- ahead of the wait for the packed bundle
gb25_status stage_own_columns(gb25_model* m, bool head_only) {
  const Grid& g = m->g;
  gb25_status s;
  const bool lazy = m->route.corrector_in_consumers(), wfly = m->route.kernels_carry_w();
  if (!head_only && m->route.head_is_done()) {
    // (LazyHead did the corrector's part)
  } else if (lazy) {
    if (head_only) m->route.head_done();
    if (!m->valid.colsum_valid) return fail(m, GB25_ERR_STATE, "internal: a lazy step without the column integrals of u, v");
    Timed t(m, GB25_K_CORRECTOR);
    if ((s = unswept_head(m, HeadRequest::slab_own_columns(launch_facts(m), wfly)))) return s;
  } else if ((s = corrector_impl(m, CorrectorRequest::own_columns()))) {
    return s;
  }
  if (head_only || !tendencies_split(m)) return GB25_OK;
  // y/z layers of the corrected u, v, own columns (lazy: the layers of the uncorrected ones are in place since Update)
  if (!lazy && (s = fill_halos_impl(m, FillRequest::uv(Columns::Own)))) return s;
  if (!wfly && (s = compute_w_impl(m, Pass::Interior))) return s;
  HIPCHK(hipStreamWaitEvent(m->stream, m->ev_join, 0));       // the own columns' pressure differences (side stream)
  return momentum_impl(m, Pass::Interior);
}

// StripsOnComm (issued on the exchange stream behind the unpack of Bundle): the two pressure strips: T, S of the halo columns are
// in; the interior pass of Update (side stream: event ev_join) must be over -- the west strip redoes its column 0
gb25_status stage_strips(gb25_model* m) {
  HIPCHK(hipStreamWaitEvent(m->stream, m->ev_join, 0));
  if (gb25_status s = compute_p_impl(m, PressureBox::strips(launch_facts(m)), true)) return s;
  HIPCHK(hipEventRecord(m->ev_strips, m->stream));
  m->strips_issued = true;
  return GB25_OK;
}

// HaloRowsCorrector (2-D decomposition): Bundle has been unpacked; the corrector on the x-halo columns of the own rows, so that the
// rows that leave for the southern / northern neighbour next (BundleRows) are corrected over their whole width
// (a lazy step: the rows leave uncorrected, like the columns; the receiver makes du, dv of its halo rows itself)
gb25_status stage_halo_rows_corrector(gb25_model* m) {
  return m->route.corrector_in_consumers() ? GB25_OK : corrector_impl(m, CorrectorRequest::halo_columns());
}

// HaloColumns: Bundle has been unpacked: corrector on the x-halo columns, then update_state without any further exchange (y/z
// layers re-filled over the extended x range; w and p recomputed in the halos).
// Folded grid: first_part = up to the y/z layers, then the rows beyond the fold arrive from the partner, second_part = the rest.
gb25_status stage_halo_columns(gb25_model* m, bool first_part, bool second_part) {
  const Grid& g = m->g;
  gb25_status s;
  const bool split = tendencies_split(m), p_early = pressure_early(m);
  // (a closure's fields travel in the bundle as well and its fills follow: the strips keep their old place behind them)
  const bool strips_first = p_early && !m->catke;
  const bool lazy = m->route.corrector_in_consumers(), wfly = m->route.kernels_carry_w();
  const bool strips_done = m->strips_issued;   // (StripsOnComm ran them on the exchange stream)
  if (second_part) m->strips_issued = false;
  // west strip (redoes column 0) + east strip
  auto pressure_strips = [&] { return pressure_on_side_stream(m, PressureBox::strips(launch_facts(m))); };
  if (first_part) {
    // the two pressure strips next to the x halos start as soon as the bundle is unpacked: T, S of the halo columns arrived
    // complete (their y/z layers were filled by their owner before it packed them), and the side stream runs them behind the
    // interior pass of Update -- beside the corrector, the fills and w of the edge strips instead of after them
    if (strips_first && !strips_done && (s = pressure_strips())) return s;
    if (lazy) {
      // du, dv of the x halo columns: the neighbours' column integrals came with the bundle, the new U, V of those columns
      // from the widened sub-cycle; their y/z layers of u, v arrived filled -- nothing else to do
      if (!m->valid.halo_colsum_valid) return fail(m, GB25_ERR_STATE, "internal: a lazy step without the neighbours' column integrals");
      // 2-D decomposition: everything at once (the bottom / top layers of the halo rows, which arrived with their interior levels: the
      // fill below); a slab: the two halo strips
      const LaunchFacts f = launch_facts(m);
      if ((s = unswept_head(m, m->Ry > 1 ? HeadRequest::mesh_rank(f, wfly) : HeadRequest::slab_halo_strips(f, wfly)))) return s;
    } else if (m->Ry == 1 && (s = corrector_impl(m, CorrectorRequest::halo_columns()))) {   // (2-D decomposition: done in HaloRowsCorrector)
      return s;
    }
    // (with the early strips T and S are left alone here: their layers are in place, own columns since Update)
    if (p_early && !strips_first) HIPCHK(hipStreamWaitEvent(m->stream, m->ev_join, 0));   // (the interior pass reads T, S)
    const FillRequest arrived{strips_first ? Fields3::UV : Fields3::UV | Fields3::TS, Fields2::Prognostic, Columns::Extended};
    if (!(lazy && strips_first) && (s = fill_halos_impl(m, arrived))) return s;
    if (!second_part) return GB25_OK;
  }
  if (p_early && !strips_first && (s = pressure_strips())) return s;   // (beside w)
  if (!wfly && (s = compute_w_impl(m, split ? Pass::Edges : Pass::Whole))) return s;
  if (strips_done) {
    HIPCHK(hipStreamWaitEvent(m->stream, m->ev_strips, 0));
  } else if (p_early) {
    HIPCHK(hipStreamWaitEvent(m->stream, m->ev_join, 0));
  } else {
    if ((s = compute_p_impl(m, PressureBox::whole(launch_facts(m))))) return s;
  }
  return momentum_impl(m, split ? Pass::Edges : Pass::Whole);
}

// Tracers: the tracer tendencies; the look-ahead of the next sub-cycle (BaroWideAhead, SubcycleAhead) runs beside them
gb25_status stage_tracers(gb25_model* m) {
  if (gb25_status s = tracers_impl(m)) return s;
  if (m->catke) return catke_step_local(m);   // (the rest after the halos of the new e and J^b: CatkeFinish)
  return atmosphere_ocean_fluxes_impl(m);
}
// CatkeFinish: the Catke groups have been unpacked -- the diffusivities and the slow tendency of e, then the fluxes
gb25_status stage_catke_finish(gb25_model* m) {
  if (gb25_status s = catke_finish_local(m)) return s;
  return atmosphere_ocean_fluxes_impl(m);
}

gb25_status slab_stage(gb25_model* m, Stage stage, int euler) {
  switch (stage) {
    case Stage::Update: return stage_update(m, euler);
    case Stage::Subcycle: return stage_subcycle(m, false, false);
    case Stage::SubcycleAhead: return stage_subcycle(m, true, false);
    case Stage::SubcycleSubsteps: return stage_subcycle(m, false, true);
    case Stage::SubcycleAheadSubsteps: return stage_subcycle(m, true, true);
    case Stage::OwnColumns: return stage_own_columns(m, false);
    case Stage::LazyHead: return stage_own_columns(m, true);
    case Stage::StripsOnComm: return stage_strips(m);
    case Stage::HaloRowsCorrector: return stage_halo_rows_corrector(m);
    case Stage::HaloColumns: return stage_halo_columns(m, true, true);
    case Stage::HaloColumnsToLayers: return stage_halo_columns(m, true, false);
    case Stage::HaloColumnsRest: return stage_halo_columns(m, false, true);
    case Stage::Tracers: return stage_tracers(m);
    case Stage::CatkeFinish: return stage_catke_finish(m);
  }
  return fail(m, GB25_ERR_INVALID_ARGUMENT, "unknown stage %d", (int)stage);
}

gb25_status update_state_local_impl(gb25_model* m) {   // update_state! without the x-halo fill
  gb25_status s;
  if ((s = mask_impl(m))) return s;   // (own columns; the halo columns arrived masked by their owners)
  if ((s = fill_halos_impl(m, FillRequest::everything(m->slab ? Columns::Extended : Columns::Own)))) return s;
  if ((s = compute_w_impl(m))) return s;
  if ((s = compute_p_impl(m, PressureBox::whole(launch_facts(m))))) return s;
  if ((s = momentum_impl(m))) return s;
  if ((s = tracers_impl(m))) return s;
  return m->catke ? catke_step_local(m) : GB25_OK;   // (the sequencer goes on with the Catke groups and catke_finish_local)
}

// ---- sequencing ------------------------------------------------------------------------------------------------------
// Everything a step of the slabs driven by this process does, in issue order, on the streams Main, Comm (the exchanges: packs,
// transfers, unpacks) and Sub (slab_protocol.hpp); record(slot, stream) marks everything issued so far on a stream, wait(slot,
// stream) makes a stream wait for that mark.  No host synchronisation anywhere.
struct StepOps {
  virtual ~StepOps() {}
  virtual int n() const = 0;
  virtual gb25_status stage(int s, Stage stage, int euler, StreamId on) = 0;
  virtual gb25_status pack(int s, Group group, StreamId on) = 0;
  virtual gb25_status unpack(int s, Group group, StreamId on) = 0;
  virtual gb25_status exchange(Group group, StreamId on) = 0;   // every slab's packs -> its neighbours' receive buffers
  virtual gb25_status local(int s, LocalOp what) = 0;
  virtual bool velocities_ready(int s) = 0;
  virtual bool subcycle_adopted(int s) = 0;
  virtual bool coupled() { return false; }   // a prescribed atmosphere is set (data-free forcing)
  virtual bool catke() { return false; }     // closure = CATKE: the halos of the new e, J^b travel inside update_state! (the Catke groups)
  virtual bool folded() = 0;          // zipper fold: exchanges with the partner rank (the groups of Peer::FoldPartner)
  virtual bool lazy() { return false; }     // this step keeps the corrector inside its consumers (known after stage Update)
  // the bundle is unpacked on the exchange stream right behind its transfer (halo columns only: nothing the main stream touches
  // before it waits for HaloColumnsArrived); on plain x slabs the two pressure strips next to the x halos follow it there
  // (StripsOnComm) -- beside the interior momentum pass instead of in front of the edge pass
  virtual bool early_unpack() { return false; }
  virtual bool early_strips() { return false; }
  virtual bool mesh_y() { return false; }   // 2-D decomposition: y halos from the southern / northern neighbour (the groups of Peer::Rows)
  virtual gb25_status record(EventSlot slot, StreamId on) = 0;
  virtual gb25_status wait(EventSlot slot, StreamId waiter) = 0;
};
#define SEQ(call)            \
  do {                       \
    gb25_status st_ = (call); \
    if (st_) return st_;     \
  } while (0)
#define EACH(expr)                         \
  for (int s = 0; s < n; s++) SEQ(expr)

// closure = CATKE: e was stepped and J^b filtered on the own columns; their halos, then the second half of compute_diffusivities!
// and the slow tendency of e (`finish`: stage CatkeFinish, or CatkeFinishLocal inside first_time_step!)
gb25_status sequence_catke_halos(StepOps& o, int n) {
  EACH(o.pack(s, Group::CatkeColumns, Main));
  SEQ(o.exchange(Group::CatkeColumns, Main));
  EACH(o.unpack(s, Group::CatkeColumns, Main));
  if (o.mesh_y()) {       // whole rows, with the x halo columns just received (the corners)
    EACH(o.pack(s, Group::CatkeRows, Main));
    SEQ(o.exchange(Group::CatkeRows, Main));
    EACH(o.unpack(s, Group::CatkeRows, Main));
  }
  if (o.folded()) {
    EACH(o.pack(s, Group::CatkeFold, Main));
    SEQ(o.exchange(Group::CatkeFold, Main));
    EACH(o.unpack(s, Group::CatkeFold, Main));
  }
  return GB25_OK;
}
gb25_status sequence_time_step(StepOps& o, int euler, bool& lookahead_in_flight) {
  const int n = o.n();
  // The previous step may have left the look-ahead chain (BaroWideAhead, SubcycleAhead) running on the other streams.  Update
  // touches nothing of it on the device (the adoption of eta, U, V is a pointer exchange on the host; its kernels update and fill
  // u, v, T, S and start the pressure), so it does not wait: on a narrow slab the chain (an exchange + the sub-cycle,
  // ~230 us) outlasts the tracer kernel it runs beside (~120 us), and Update fills part of the difference.
  const bool in_flight = lookahead_in_flight;
  lookahead_in_flight = false;
  EACH(o.stage(s, Stage::Update, euler, Main));
  bool adopted = true;         // the sub-cycle of this step is already done
  for (int s = 0; s < n; s++) adopted = adopted && o.subcycle_adopted(s);
  if (in_flight && !adopted)   // not adopted after all: it must be over before its buffers and work arrays are reused
    SEQ(o.wait(ChainEnd, Main));
  SEQ(o.record(UpdateWritten, Main));
  if (!adopted) {
    // The small barotropic exchange is on the critical path and is posted FIRST: the point-to-point transfers of one
    // communicator run in posting order, so the 6 MB bundle must not be queued ahead of it.
    EACH(o.pack(s, Group::BaroWide, Main));
    SEQ(o.exchange(Group::BaroWide, Main));
  }
  SEQ(o.wait(UpdateWritten, Comm));        // the 3-D bundle leaves on the second stream ...
  EACH(o.pack(s, Group::Bundle, Comm));
  SEQ(o.record(BundlePacked, Comm));
  SEQ(o.exchange(Group::Bundle, Comm));
  const bool early = o.early_unpack();
  if (early)
    for (int s = 0; s < n; s++) {
      SEQ(o.unpack(s, Group::Bundle, Comm));
      if (o.early_strips()) SEQ(o.stage(s, Stage::StripsOnComm, euler, Comm));
    }
  // 2-D decomposition, a step that keeps the corrector inside its consumers: the rows leave as they are (HaloRowsCorrector has
  // nothing to do), so their exchange follows the bundle on the exchange stream instead of waiting for the main stream to get there
  // (one cross-stream hop less: 0.538 -> 0.504 ms per step of a 360 x 360 rank, tools/slab_selfring.py --mesh 4 2)
  const bool rows_early = early && o.mesh_y() && o.lazy();
  if (rows_early) {
    EACH(o.pack(s, Group::BundleRows, Comm));
    SEQ(o.exchange(Group::BundleRows, Comm));
    EACH(o.unpack(s, Group::BundleRows, Comm));
  }
  if (!adopted && (o.folded() || o.mesh_y())) {
    // zipper fold: the work arrays are tall as well as wide.  Once every slab has its wide halo columns, the rows south of
    // the pivot row go to the partner rank P-1-r (FoldTall) and become its image rows beyond the pivot row; then the substeps
    // run with no further exchange.  2-D decomposition: likewise the W rows next to an open side go to the southern /
    // northern neighbour (BaroWideRows), with the wide halo columns just received: the corners
    for (int s = 0; s < n; s++) {
      SEQ(o.unpack(s, Group::BaroWide, Main));
      SEQ(o.stage(s, Stage::Subcycle, euler, Main));      // (the interior copy only)
      if (o.mesh_y()) SEQ(o.pack(s, Group::BaroWideRows, Main));
      if (o.folded()) SEQ(o.pack(s, Group::FoldTall, Main));
    }
    if (o.mesh_y()) SEQ(o.exchange(Group::BaroWideRows, Main));
    if (o.folded()) SEQ(o.exchange(Group::FoldTall, Main));
    for (int s = 0; s < n; s++) {
      if (o.mesh_y()) SEQ(o.unpack(s, Group::BaroWideRows, Main));
      if (o.folded()) SEQ(o.unpack(s, Group::FoldTall, Main));
      SEQ(o.stage(s, Stage::SubcycleSubsteps, euler, Main));
    }
  } else if (!adopted) {       // ... and is in flight while the sub-cycle runs here (it leaves the x halo columns of the
    for (int s = 0; s < n; s++) {   // new eta, U, V behind as well: the slab is widened by Ns + 1 + H columns, no BaroHalo)
      SEQ(o.unpack(s, Group::BaroWide, Main));
      SEQ(o.stage(s, Stage::Subcycle, euler, Main));
    }
  }
  if (o.lazy()) {
    // the corrector inside its consumers writes nothing the bundle is packed from: du, dv and the chunk bases of w of the own
    // columns (LazyHead) need the adopted sub-cycle only; the interior momentum pass, which overwrites chunk sums the bundle
    // carries, waits for the pack
    if (in_flight && adopted) SEQ(o.wait(ChainEnd, Main));
    EACH(o.stage(s, Stage::LazyHead, euler, Main));
    SEQ(o.wait(BundlePacked, Main));
  } else {
    SEQ(o.wait(BundlePacked, Main));   // the corrector rewrites the columns the bundle was packed from
    if (in_flight && adopted)          // ... and reads the adopted sub-cycle: the look-ahead chain has finished (ChainEnd sits
      SEQ(o.wait(ChainEnd, Main));     // behind the chain, ahead of this step's bundle on the same stream)
  }
  EACH(o.stage(s, Stage::OwnColumns, euler, Main));   // own columns + interior tendencies, while the exchanges are in flight
  SEQ(o.record(HaloColumnsArrived, Comm));
  SEQ(o.wait(HaloColumnsArrived, Main));
  if (o.mesh_y() && !rows_early) {
    // 2-D decomposition: the H rows next to an open side, with the x halo columns just received (the corners)
    for (int s = 0; s < n; s++) {
      if (!early) SEQ(o.unpack(s, Group::Bundle, Main));
      SEQ(o.stage(s, Stage::HaloRowsCorrector, euler, Main));   // (the rows leave corrected)
      SEQ(o.pack(s, Group::BundleRows, Main));
    }
    SEQ(o.exchange(Group::BundleRows, Main));
    EACH(o.unpack(s, Group::BundleRows, Main));
  }
  if (o.folded()) {
    // the rows beyond the fold come from the partner once every slab has its x halos and y/z layers (the partner sends
    // its halo columns too: the corners), then the rest of update_state!
    for (int s = 0; s < n; s++) {
      if (!o.mesh_y() && !early) SEQ(o.unpack(s, Group::Bundle, Main));
      SEQ(o.stage(s, Stage::HaloColumnsToLayers, euler, Main));
      SEQ(o.pack(s, Group::FoldBundle, Main));
    }
    SEQ(o.exchange(Group::FoldBundle, Main));
    for (int s = 0; s < n; s++) {
      SEQ(o.unpack(s, Group::FoldBundle, Main));
      SEQ(o.stage(s, Stage::HaloColumnsRest, euler, Main));
    }
  } else {
    for (int s = 0; s < n; s++) {
      if (!o.mesh_y() && !early) SEQ(o.unpack(s, Group::Bundle, Main));
      SEQ(o.stage(s, Stage::HaloColumns, euler, Main));
    }
  }
  // the next step's G.U, G.V exist now: its wide-halo exchange and sub-cycle run on the other streams beside the tracer tendencies
  bool ready = true;
  for (int s = 0; s < n; s++) ready = ready && o.velocities_ready(s);
  if (ready) {
    SEQ(o.record(NextTendenciesExist, Main));
    SEQ(o.wait(NextTendenciesExist, Comm));
    EACH(o.pack(s, Group::BaroWideAhead, Comm));
    SEQ(o.exchange(Group::BaroWideAhead, Comm));
    if (o.folded() || o.mesh_y()) {
      for (int s = 0; s < n; s++) {
        SEQ(o.unpack(s, Group::BaroWideAhead, Comm));
        SEQ(o.stage(s, Stage::SubcycleAhead, euler, Comm));    // (the interior copy only)
        if (o.mesh_y()) SEQ(o.pack(s, Group::BaroWideRowsAhead, Comm));
        if (o.folded()) SEQ(o.pack(s, Group::FoldTall, Comm));
      }
      // the neighbours' rows / the image rows beyond the pivot row, then the substeps on their own stream
      if (o.mesh_y()) SEQ(o.exchange(Group::BaroWideRowsAhead, Comm));
      if (o.folded()) SEQ(o.exchange(Group::FoldTall, Comm));
      for (int s = 0; s < n; s++) {
        if (o.mesh_y()) SEQ(o.unpack(s, Group::BaroWideRowsAhead, Comm));
        if (o.folded()) SEQ(o.unpack(s, Group::FoldTall, Comm));
      }
      SEQ(o.record(ChainExchanged, Comm));
      SEQ(o.wait(ChainExchanged, Sub));
      EACH(o.stage(s, Stage::SubcycleAheadSubsteps, euler, Sub));
    } else {
      EACH(o.unpack(s, Group::BaroWideAhead, Comm));
      SEQ(o.record(ChainExchanged, Comm));
      SEQ(o.wait(ChainExchanged, Sub));
      EACH(o.stage(s, Stage::SubcycleAhead, euler, Sub));     // (x halo columns of the new eta, U, V included: nothing to exchange after it)
    }
    SEQ(o.record(ChainEnd, Sub));
    lookahead_in_flight = true;
  }
  EACH(o.stage(s, Stage::Tracers, euler, Main));
  if (o.catke()) {
    SEQ(sequence_catke_halos(o, n));
    EACH(o.stage(s, Stage::CatkeFinish, euler, Main));
  }
  return GB25_OK;
}
// first_time_step!: initialize!, update_state!, then an Euler step (GB-25 src/timestepping_utils.jl:21-27)
gb25_status sequence_first_time_step(StepOps& o, bool& lookahead_in_flight) {
  const int n = o.n();
  if (lookahead_in_flight) {
    SEQ(o.wait(ChainEnd, Main));             // (the chain's last launches, on the sub stream)
    SEQ(o.record(HaloColumnsArrived, Comm));
    SEQ(o.wait(HaloColumnsArrived, Main));
    lookahead_in_flight = false;
  }
  for (int s = 0; s < n; s++) {
    SEQ(o.local(s, Initialize));
    SEQ(o.local(s, FillLocal));
    SEQ(o.pack(s, Group::Bundle, Main));
    SEQ(o.pack(s, Group::BaroHalo, Main));
  }
  SEQ(o.exchange(Group::Bundle, Main));
  SEQ(o.exchange(Group::BaroHalo, Main));
  if (o.mesh_y()) {
    for (int s = 0; s < n; s++) {
      SEQ(o.unpack(s, Group::Bundle, Main));
      SEQ(o.unpack(s, Group::BaroHalo, Main));
      SEQ(o.pack(s, Group::BundleRows, Main));
      SEQ(o.pack(s, Group::BaroHaloRows, Main));
    }
    SEQ(o.exchange(Group::BundleRows, Main));
    SEQ(o.exchange(Group::BaroHaloRows, Main));
    for (int s = 0; s < n; s++) {
      SEQ(o.unpack(s, Group::BundleRows, Main));
      SEQ(o.unpack(s, Group::BaroHaloRows, Main));
    }
  }
  if (o.folded()) {
    for (int s = 0; s < n; s++) {
      if (!o.mesh_y()) {
        SEQ(o.unpack(s, Group::Bundle, Main));
        SEQ(o.unpack(s, Group::BaroHalo, Main));
      }
      SEQ(o.local(s, MaskFillLocal));
      SEQ(o.pack(s, Group::FoldBundle, Main));
    }
    SEQ(o.exchange(Group::FoldBundle, Main));
    for (int s = 0; s < n; s++) {
      SEQ(o.unpack(s, Group::FoldBundle, Main));
      SEQ(o.local(s, AuxiliariesTendenciesLocal));
    }
  } else {
    for (int s = 0; s < n; s++) {
      if (!o.mesh_y()) {
        SEQ(o.unpack(s, Group::Bundle, Main));
        SEQ(o.unpack(s, Group::BaroHalo, Main));
      }
      SEQ(o.local(s, UpdateStateLocal));
    }
  }
  if (o.catke()) {
    SEQ(sequence_catke_halos(o, n));
    EACH(o.local(s, CatkeFinishLocal));
  }
  if (o.coupled()) {
    // a coupled model (data-free forcing) updates its state at iteration 0: the atmosphere-ocean fluxes of the initial state,
    // then the tendencies (and, with CATKE, another compute_diffusivities!) that see them
    EACH(o.local(s, FirstFluxesLocal));
    EACH(o.local(s, TendenciesLocal));
    if (o.catke()) {
      SEQ(sequence_catke_halos(o, n));
      EACH(o.local(s, CatkeFinishLocal));
    }
  }
  return sequence_time_step(o, 1, lookahead_in_flight);
}
#undef EACH
#undef SEQ

// Dry run: records the operations instead of launching anything (no HIP call) -- how the CPU-only tests see the order.
struct TraceOps : StepOps {
  int nslabs;
  bool adopted, ready;
  std::string log;
  bool fold = false, is_coupled = false, mesh = false, is_lazy = false, early = false, is_catke = false;
  TraceOps(int n_, bool a, bool r) : nslabs(n_), adopted(a), ready(r) {}
  bool folded() override { return fold; }
  bool mesh_y() override { return mesh; }
  bool lazy() override { return is_lazy; }
  bool early_unpack() override { return early; }
  bool early_strips() override { return early && !fold && !mesh; }
  bool coupled() override { return is_coupled; }
  bool catke() override { return is_catke; }
  void add(const char* fmt, ...) {
    char buf[96];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    log += buf;
    log += '\n';
  }
  static const char* st(StreamId on) { return kStreamNames[on]; }
  int n() const override { return nslabs; }
  gb25_status stage(int s, Stage stage, int euler, StreamId c) override { add("stage %d slab %d euler %d %s", stage, s, euler, st(c)); return GB25_OK; }
  gb25_status pack(int s, Group group, StreamId c) override { add("pack %d slab %d %s", group, s, st(c)); return GB25_OK; }
  gb25_status unpack(int s, Group group, StreamId c) override { add("unpack %d slab %d %s", group, s, st(c)); return GB25_OK; }
  gb25_status exchange(Group group, StreamId c) override { add("exchange %d %s", group, st(c)); return GB25_OK; }
  gb25_status local(int s, LocalOp what) override { add("%s slab %d main", kLocalOpNames[what], s); return GB25_OK; }
  bool velocities_ready(int) override { return ready; }
  bool subcycle_adopted(int) override { return adopted; }
  gb25_status record(EventSlot slot, StreamId c) override { add("record %d %s", slot, st(c)); return GB25_OK; }
  gb25_status wait(EventSlot slot, StreamId waiter) override { add("wait %d %s", slot, st(waiter)); return GB25_OK; }
};

// ---- transports ------------------------------------------------------------------------------------------------------
struct Transport {
  virtual ~Transport() {}
  // buffer set b, nbytes per side, on stream st
  virtual gb25_status exchange(SlabGroup& G, BufferSet b, size_t nbytes, hipStream_t st) = 0;
  virtual const char* name() const = 0;
};

}  // namespace

// The slabs this process drives, their exchange buffers, the second stream and the transport.
struct SlabGroup {
  std::vector<gb25_model*> slabs;
  hipStream_t main = nullptr, comm = nullptr, sub = nullptr;   // (sub: the substeps of the sub-cycle look-ahead)
  hipEvent_t ev[NSLOTS] = {};
  // everything the second and third stream hold is over (host writes, grid changes, collective setters)
  hipError_t sync_side() {
    hipError_t e = comm ? hipStreamSynchronize(comm) : hipSuccess;
    if (e == hipSuccess && sub) e = hipStreamSynchronize(sub);
    return e;
  }
  Transport* transport = nullptr;
  // [slab][buffer set][side]: 0 west, 1 east (Peer::Ring); 0 south, 1 north (Peer::Rows); side 0 only (Peer::FoldPartner)
  std::vector<std::array<std::array<real*, 2>, NSETS>> send, recv;
  size_t elems[NSETS] = {};      // elements per side of buffer set b in an exchange
  size_t capacity[NSETS] = {};   // ... and allocated
  bool lookahead_in_flight = false;
  // neighbour handshake of the collective mutators (see collective_guard)
  unsigned long long *tok_dev = nullptr, *tok_host = nullptr;
};

namespace {

// rank = ry Rx + rx: the ring neighbours within the row, the neighbours in the column, the fold partner within the top row
struct MeshPos {
  int Rx, Ry, rx, ry;
  explicit MeshPos(const gb25_model* m) : Rx(m->Rx), Ry(m->Ry), rx(m->rx), ry(m->ry) {}
  MeshPos(int Rx_, int Ry_, int rank) : Rx(Rx_), Ry(Ry_), rx(rank % Rx_), ry(rank / Rx_) {}
  int west() const { return ry * Rx + (rx + Rx - 1) % Rx; }
  int east() const { return ry * Rx + (rx + 1) % Rx; }
  int south() const { return ry > 0 ? (ry - 1) * Rx + rx : -1; }
  int north() const { return ry < Ry - 1 ? (ry + 1) * Rx + rx : -1; }
  int partner() const { return ry * Rx + (Rx - 1 - rx); }
};

// several slabs of one decomposition in this process, all on one device: a ring of device-to-device copies
struct LocalRingTransport : Transport {
  const char* name() const override { return "local"; }
  gb25_status exchange(SlabGroup& G, BufferSet b, size_t nbytes, hipStream_t st) override {
    const int P = (int)G.slabs.size();
    for (int r = 0; r < P; r++) {
      gb25_model* m = G.slabs[r];
      const MeshPos q(m);
      const Peer peer = set_info(b).peer;
      if (peer == Peer::FoldPartner) {   // zipper fold: slab rx <-> slab Rx-1-rx of the top row (the middle slab of an odd count is its own partner)
        if (m->g.cv.north_fold) HIPCHK(hipMemcpyAsync(G.recv[q.partner()][b][0], G.send[r][b][0], nbytes, hipMemcpyDeviceToDevice, st));
      } else if (peer == Peer::Rows) {    // my southern pack -> the southern neighbour's northern halo; my northern pack -> ... southern halo
        if (q.south() >= 0) HIPCHK(hipMemcpyAsync(G.recv[q.south()][b][1], G.send[r][b][0], nbytes, hipMemcpyDeviceToDevice, st));
        if (q.north() >= 0) HIPCHK(hipMemcpyAsync(G.recv[q.north()][b][0], G.send[r][b][1], nbytes, hipMemcpyDeviceToDevice, st));
      } else {                  // my west pack -> west neighbour's east halo; my east pack -> east neighbour's west halo
        HIPCHK(hipMemcpyAsync(G.recv[q.west()][b][1], G.send[r][b][0], nbytes, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(G.recv[q.east()][b][0], G.send[r][b][1], nbytes, hipMemcpyDeviceToDevice, st));
      }
    }
    return GB25_OK;
  }
};

// librccl, resolved at run time.  When the host process has RCCL loaded already (PyTorch-ROCm ships one with the same
// soname) dlopen hands back that copy, so there is exactly one RCCL in the process.
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string error;
  bool load() {
    if (lib) return true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) {
      error = std::string("librccl.so.1 could not be loaded: ") + dlerror();
      return false;
    }
    auto sym = [&](const char* n) {
      void* p = dlsym(lib, n);
      if (!p) error = std::string("librccl lacks ") + n;
      return p;
    };
    GetUniqueId = (decltype(GetUniqueId))sym("ncclGetUniqueId");
    CommInitRank = (decltype(CommInitRank))sym("ncclCommInitRank");
    CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
    CommCount = (decltype(CommCount))sym("ncclCommCount");
    Send = (decltype(Send))sym("ncclSend");
    Recv = (decltype(Recv))sym("ncclRecv");
    GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
    GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
    GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
    if (!GetUniqueId || !CommInitRank || !CommDestroy || !CommCount || !Send || !Recv || !GroupStart || !GroupEnd || !GetErrorString) {
      lib = nullptr;
      return false;
    }
    return true;
  }
};
RcclApi& rccl() {
  static RcclApi api;
  return api;
}
#define NCCLCHK(call)                                                                                             \
  do {                                                                                                            \
    ncclResult_t r_ = (call);                                                                                     \
    if (r_ != ncclSuccess)                                                                                        \
      return fail(m, GB25_ERR_COMM, "%s:%d: %s failed: %s", __FILE__, __LINE__, #call, rccl().GetErrorString(r_)); \
  } while (0)

// What one rank posts inside ONE ncclGroup for buffer set b, in posting order: (send?, peer rank, side of the buffer set).  The
// single place that knows the protocol -- RcclTransport::exchange posts exactly this, gb25_debug_exchange_plan prints it, and the
// CPU tests prove from it that every rank's ordered sends to a peer mirror that peer's ordered receives (tests/test_distributed_cpu.py).
struct PlanOp { bool send; int peer; int side; };
inline std::vector<PlanOp> exchange_plan(const MeshPos& q, bool north_fold, Peer peer) {
  std::vector<PlanOp> p;
  if (peer == Peer::Rows) { // 2-D decomposition: the southern and the northern neighbour, where they exist
    if (q.south() >= 0) p.push_back({true, q.south(), 0});
    if (q.north() >= 0) p.push_back({true, q.north(), 1});
    if (q.north() >= 0) p.push_back({false, q.north(), 1});
    if (q.south() >= 0) p.push_back({false, q.south(), 0});
  } else if (peer == Peer::FoldPartner) {   // zipper fold: the partner is the mirrored rank of the (top) row; a rank that is its own partner copies
    const int self = q.ry * q.Rx + q.rx;
    if (north_fold && q.partner() != self) {
      p.push_back({true, q.partner(), 0});
      p.push_back({false, q.partner(), 0});
    }
  } else {                  // the ring: sends [west pack, east pack], receives [east halo, west halo]
    p.push_back({true, q.west(), 0});
    p.push_back({true, q.east(), 1});
    p.push_back({false, q.east(), 1});
    p.push_back({false, q.west(), 0});
  }
  return p;
}

// one slab per process, one process per GPU: the ring neighbours are ranks rank-1 and rank+1 of the communicator.
// Posting order is part of the protocol: sends [west pack, east pack], receives [east halo, west halo].  With two
// ranks both neighbours are the same peer and the messages of one pair match in posting order, so the peer's FIRST send
// (its west pack) must meet our FIRST receive (our east halo); with one rank (the self-ring) likewise.
struct RcclTransport : Transport {
  ncclComm_t comm = nullptr;
  int rank = 0, nranks = 1;
  // rehearsal of ONE rank of a decomposition alone on one device (tools/slab_selfring.py --mesh): a communicator of size one, every
  // neighbour is the rank itself -- the messages of a group match in posting order, so a southern pack lands in the northern halo
  bool alone = false;
  int peer(int r) const { return alone ? 0 : r; }
  const char* name() const override { return "rccl"; }
  ~RcclTransport() override {
    if (comm) rccl().CommDestroy(comm);
  }
  gb25_status send_recv(gb25_model* m, const void* sw, const void* se, void* rw, void* re, size_t nbytes, hipStream_t st) {
    const MeshPos q(m);
    const int west = peer(q.west()), east = peer(q.east());
    RcclApi& R = rccl();
    NCCLCHK(R.GroupStart());
    NCCLCHK(R.Send(sw, nbytes, ncclInt8, west, comm, st));
    NCCLCHK(R.Send(se, nbytes, ncclInt8, east, comm, st));
    NCCLCHK(R.Recv(re, nbytes, ncclInt8, east, comm, st));
    NCCLCHK(R.Recv(rw, nbytes, ncclInt8, west, comm, st));
    NCCLCHK(R.GroupEnd());
    return GB25_OK;
  }
  gb25_status exchange(SlabGroup& G, BufferSet b, size_t nbytes, hipStream_t st) override {
    gb25_model* m = G.slabs[0];
    const MeshPos q(m);
    const Peer to = set_info(b).peer;
    if (to == Peer::FoldPartner) {
      if (!m->g.cv.north_fold) return GB25_OK;
      if (q.partner() == rank || alone) {   // (its own partner: the middle slab of an odd count, the self-ring)
        HIPCHK(hipMemcpyAsync(G.recv[0][b][0], G.send[0][b][0], nbytes, hipMemcpyDeviceToDevice, st));
        return GB25_OK;
      }
    }
    const std::vector<PlanOp> plan = exchange_plan(q, m->g.cv.north_fold != 0, to);
    if (plan.empty()) return GB25_OK;
    RcclApi& R = rccl();
    NCCLCHK(R.GroupStart());
    for (const PlanOp& op : plan) {
      if (op.send) NCCLCHK(R.Send(G.send[0][b][op.side], nbytes, ncclInt8, peer(op.peer), comm, st));
      else NCCLCHK(R.Recv(G.recv[0][b][op.side], nbytes, ncclInt8, peer(op.peer), comm, st));
    }
    NCCLCHK(R.GroupEnd());
    return GB25_OK;
  }
};

// the host moves the buffers (synchronous): rehearsal of the multi-process path where RCCL cannot run
struct CallbackTransport : Transport {
  gb25_exchange_fn fn = nullptr;
  void* user = nullptr;
  const char* name() const override { return "callback"; }
  gb25_status exchange(SlabGroup& G, BufferSet b, size_t nbytes, hipStream_t st) override {
    gb25_model* m = G.slabs[0];
    HIPCHK(hipStreamSynchronize(st));   // the packs are complete
    // (Peer::FoldPartner: to and from the fold partner rank P-1-r; the east pointers are null)
    // (Peer::Rows: to and from the southern [west pointers] and northern [east pointers] neighbour of a 2-D decomposition; null
    // where there is none)
    const Peer peer = set_info(b).peer;
    if (peer == Peer::FoldPartner && !m->g.cv.north_fold) return GB25_OK;
    int rc;
    if (peer == Peer::FoldPartner) rc = fn(user, b, G.send[0][b][0], nullptr, G.recv[0][b][0], nullptr, (int64_t)nbytes);
    else if (peer == Peer::Rows) rc = fn(user, b, m->ys_open ? G.send[0][b][0] : nullptr, m->yn_open ? G.send[0][b][1] : nullptr,
                             m->ys_open ? G.recv[0][b][0] : nullptr, m->yn_open ? G.recv[0][b][1] : nullptr, (int64_t)nbytes);
    else rc = fn(user, b, G.send[0][b][0], G.send[0][b][1], G.recv[0][b][0], G.recv[0][b][1], (int64_t)nbytes);
    if (rc != 0) return fail(m, GB25_ERR_COMM, "the host's exchange callback failed with code %d (buffer set %d)", rc, b);
    return GB25_OK;
  }
};

// the real StepOps: the slabs of a SlabGroup
struct GroupOps : StepOps {
  SlabGroup& G;
  explicit GroupOps(SlabGroup& g_) : G(g_) {}
  int n() const override { return (int)G.slabs.size(); }
  hipStream_t st(StreamId on) const { return on == Sub ? G.sub : on == Comm ? G.comm : G.main; }
  gb25_status stage(int s, Stage stage, int euler, StreamId c) override {
    OnStream on(G.slabs[s], st(c));
    return slab_stage(G.slabs[s], stage, euler);
  }
  bool folded() override {   // (2-D decomposition: the top row of ranks only; the others skip the partner's groups)
    for (gb25_model* m : G.slabs)
      if (m->g.cv.north_fold) return true;
    return false;
  }
  bool mesh_y() override { return G.slabs[0]->Ry > 1; }
  bool lazy() override {
    for (gb25_model* m : G.slabs)
      if (!m->route.corrector_in_consumers()) return false;
    return true;
  }
  bool early_unpack() override {
    for (gb25_model* m : G.slabs)
      if (!m->early_strips || !m->two_streams) return false;
    return true;
  }
  bool early_strips() override {
    for (gb25_model* m : G.slabs)
      if (!strips_on_comm(m)) return false;
    return true;
  }
  bool coupled() override { return G.slabs[0]->coupled; }
  bool catke() override { return G.slabs[0]->catke; }
  gb25_status move(int s, Group group, StreamId c, bool pack) {
    gb25_model* m = G.slabs[s];
    OnStream on(m, st(c));
    const GroupInfo& info = group_info(group);
    const std::array<real*, 2>& buf = (pack ? G.send : G.recv)[s][info.set];
    switch (info.mover) {
      case Mover::FoldRows:
        if (!m->g.cv.north_fold) return GB25_OK;
        return pack ? fold_pack(m, buf[0], info.closure) : fold_unpack(m, buf[0], info.closure);
      case Mover::TallRows: return m->g.cv.north_fold ? tall_rows_impl(m, buf[0], pack) : GB25_OK;
      case Mover::Rows: return move_rows(m, group, buf.data(), pack);
      case Mover::Columns:
        if (pack && group == Group::Bundle) m->valid.halo_colsums_packed();   // (every slab alike: same calls, same state)
        return pack_unpack(m, group, buf.data(), pack);
    }
    return GB25_OK;
  }
  gb25_status pack(int s, Group group, StreamId c) override { return move(s, group, c, true); }
  gb25_status unpack(int s, Group group, StreamId c) override { return move(s, group, c, false); }
  gb25_status exchange(Group group, StreamId c) override {
    const BufferSet b = group_info(group).set;
    return G.transport->exchange(G, b, G.elems[b] * sizeof(real), st(c));
  }
  gb25_status local(int s, LocalOp what) override {
    gb25_model* m = G.slabs[s];
    gb25_status s_;
    switch (what) {
      case Initialize: return initialize_impl(m);
      case FillLocal: return fill_halos_impl(m, FillRequest::everything(Columns::Own));
      case UpdateStateLocal: return update_state_local_impl(m);
      case MaskFillLocal:
        if ((s_ = mask_impl(m))) return s_;
        return fill_halos_impl(m, FillRequest::everything(Columns::Extended));
      case AuxiliariesTendenciesLocal:
        if ((s_ = compute_w_impl(m))) return s_;
        if ((s_ = compute_p_impl(m, PressureBox::whole(launch_facts(m))))) return s_;
        [[fallthrough]];
      case TendenciesLocal:
        if ((s_ = momentum_impl(m))) return s_;
        if ((s_ = tracers_impl(m))) return s_;
        return m->catke ? catke_step_local(m) : GB25_OK;
      case FirstFluxesLocal: return atmosphere_ocean_fluxes_impl(m);   // coupled model, iteration 0: fluxes of the initial state
      case CatkeFinishLocal: return catke_finish_local(m);
    }
    return fail(m, GB25_ERR_INVALID_ARGUMENT, "unknown local operation %d", (int)what);
  }
  bool velocities_ready(int s) override {
    gb25_model* m = G.slabs[s];
    return m->valid.velocities_ready(m->baro_ahead);
  }
  bool subcycle_adopted(int s) override { return G.slabs[s]->baro_adopted; }
  gb25_status record(EventSlot slot, StreamId c) override {
    gb25_model* m = G.slabs[0];
    HIPCHK(hipEventRecord(G.ev[slot], st(c)));
    return GB25_OK;
  }
  gb25_status wait(EventSlot slot, StreamId waiter) override {
    gb25_model* m = G.slabs[0];
    HIPCHK(hipStreamWaitEvent(st(waiter), G.ev[slot], 0));
    return GB25_OK;
  }
};

void group_destroy(SlabGroup* G) {
  if (!G) return;
  G->sync_side();
  if (G->main) hipStreamSynchronize(G->main);
  delete G->transport;
  for (auto& s : G->send)
    for (auto& b : s)
      for (real* p : b)
        if (p) hipFree(p);
  for (auto& s : G->recv)
    for (auto& b : s)
      for (real* p : b)
        if (p) hipFree(p);
  for (hipEvent_t e : G->ev)
    if (e) hipEventDestroy(e);
  if (G->comm) hipStreamDestroy(G->comm);
  if (G->sub) hipStreamDestroy(G->sub);
  if (G->tok_dev) hipFree(G->tok_dev);
  if (G->tok_host) hipHostFree(G->tok_host);
  for (gb25_model* m : G->slabs) {
    m->group = nullptr;
    m->stream = m->own_stream;
  }
  delete G;
}

// Elements per side of buffer set b: what the largest slab packs (2-D decomposition: the top row of ranks folds, the others do not;
// every slab gets buffers of the size a folded one needs)
size_t group_set_elems(const std::vector<gb25_model*>& slabs, BufferSet b) {
  size_t need = 0;
  for (gb25_model* q : slabs) need = std::max(need, (size_t)set_elems(q, b));
  return need;
}
// The Bundle carries more once an option adds the chunk sums of u, v to it, and a closure brings exchanges of its own (CATKE: e,
// J^b -- switched on after the context was built, its sets grow from one element): sizes again, larger buffers if needed.  Called
// at the head of the composites; every rank made the same (collective) setter calls.
gb25_status group_refresh(SlabGroup* G) {
  gb25_model* m = G->slabs[0];
  const int n = (int)G->slabs.size();
  for (BufferSet b : {SetBundle, SetFoldBundle, SetBundleRows, SetCatkeColumns, SetCatkeRows, SetCatkeFold}) {
    const size_t need = group_set_elems(G->slabs, b);
    if (need == G->elems[b]) continue;
    HIPCHK(G->sync_side());
    HIPCHK(hipStreamSynchronize(G->main));
    if (need > G->capacity[b]) {
      for (int s = 0; s < n; s++)
        for (int side = 0; side < set_sides((BufferSet)b); side++) {
          if (G->send[s][b][side]) hipFree(G->send[s][b][side]);
          if (G->recv[s][b][side]) hipFree(G->recv[s][b][side]);
          G->send[s][b][side] = G->recv[s][b][side] = nullptr;
          if (hipMalloc(&G->send[s][b][side], need * sizeof(real)) != hipSuccess ||
              hipMalloc(&G->recv[s][b][side], need * sizeof(real)) != hipSuccess)
            return fail(m, GB25_ERR_OUT_OF_MEMORY, "exchange buffers of %zu elements", need);
        }
      G->capacity[b] = need;
    }
    G->elems[b] = need;
  }
  return GB25_OK;
}

// (The comm stream is an ordinary stream.  A high-priority one -- tried so that it would not share a hardware queue with
// the slab's side stream -- made the 180-column step 2.3x slower beside RCCL's kernel.  What helps is more hardware queues
// for the process: GPU_MAX_HW_QUEUES=8, which bench.py and tools/slab_selfring.py set before the runtime starts (one model per
// process; the Python package itself leaves the runtime's default alone, see bench.py).)
// Builds the exchange context of `n` slabs (n > 1 only with the local transport).  Takes ownership of `tr`.
gb25_status group_create(gb25_model* const* slabs, int n, Transport* tr) {
  gb25_model* m = slabs[0];
  for (int s = 0; s < n; s++) {
    if (!slabs[s] || !slabs[s]->slab) {
      delete tr;
      return fail(m, GB25_ERR_STATE, "slab %d is not a slab of an x decomposition (nranks > 1 or slab_mode = 1)", s);
    }
    if (slabs[s]->group) group_destroy(slabs[s]->group);
  }
  SlabGroup* G = new SlabGroup();
  G->transport = tr;
  G->slabs.assign(slabs, slabs + n);
  G->main = m->own_stream;
  for (int s = 0; s < n; s++) {
    slabs[s]->group = G;
    slabs[s]->group_index = s;
    slabs[s]->stream = G->main;
  }
  gb25_status st = GB25_OK;
  do {
    if (hipSetDevice(m->cfg.device) != hipSuccess ||
        hipStreamCreateWithFlags(&G->comm, hipStreamNonBlocking) != hipSuccess ||
        [&]() {
          // the substeps' few blocks should not queue behind what is left of the tracer kernel's grid: highest priority
          // (option SUB_STREAM_PRIORITY = 0: an ordinary stream)
          int least = 0, greatest = 0;
          if (m->sub_priority && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
            return hipStreamCreateWithPriority(&G->sub, hipStreamNonBlocking, greatest);
          return hipStreamCreateWithFlags(&G->sub, hipStreamNonBlocking);
        }() != hipSuccess) { st = GB25_ERR_HIP; break; }
    for (auto& e : G->ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) st = GB25_ERR_HIP;
    if (st) break;
    for (int b = 0; b < NSETS; b++) G->capacity[b] = G->elems[b] = group_set_elems(G->slabs, (BufferSet)b);
    G->send.resize(n);
    G->recv.resize(n);
    for (int s = 0; s < n && !st; s++)
      for (int b = 0; b < NSETS && !st; b++)
        for (int side = 0; side < 2; side++) G->send[s][b][side] = G->recv[s][b][side] = nullptr;
    for (int s = 0; s < n && !st; s++)
      for (int b = 0; b < NSETS && !st; b++)
        for (int side = 0; side < set_sides((BufferSet)b) && !st; side++) {
          G->send[s][b][side] = G->recv[s][b][side] = nullptr;
          if (hipMalloc(&G->send[s][b][side], G->elems[b] * sizeof(real)) != hipSuccess ||
              hipMalloc(&G->recv[s][b][side], G->elems[b] * sizeof(real)) != hipSuccess)
            st = GB25_ERR_OUT_OF_MEMORY;
        }
    if (st) break;
    if (hipMalloc(&G->tok_dev, 8 * sizeof(unsigned long long)) != hipSuccess ||
        hipHostMalloc(&G->tok_host, 8 * sizeof(unsigned long long)) != hipSuccess) st = GB25_ERR_OUT_OF_MEMORY;
  } while (0);
  if (st) {
    group_destroy(G);
    return fail(m, st, "could not build the exchange context (%s)", hipGetErrorString(hipGetLastError()));
  }
  return GB25_OK;
}

// Calls that change what the look-aheads were made from (host writes, a new dt, an option, a handed-out pointer) void
// the look-aheads of the calling slab -- and, through the halo columns the neighbours hold, theirs.  On a decomposed
// model they are therefore COLLECTIVE: every rank must make the same call (as with set!(model, ...) on an Oceananigans
// Distributed grid).  With the RCCL transport the call shakes hands with both ring neighbours (16 bytes each way): a
// rank that made a different call gets GB25_ERR_STATE here instead of a mismatched exchange later, a rank that made no
// call leaves the others waiting AT the call.  The branch every rank takes in the next step (adopt the look-aheads or
// not) then depends on agreed values only.
gb25_status collective_guard(gb25_model* m, unsigned op, unsigned arg, double payload) {
  SlabGroup* G = m->group;
  if (!G) return GB25_OK;
  RcclTransport* R = dynamic_cast<RcclTransport*>(G->transport);
  if (!R) return GB25_OK;   // local slabs share one host thread; the callback transport is a rehearsal
  unsigned long long bits;
  memcpy(&bits, &payload, sizeof bits);
  unsigned long long* h = G->tok_host;
  h[0] = h[2] = ((unsigned long long)op << 32) | arg;
  h[1] = h[3] = bits;
  HIPCHK(G->sync_side());   // a look-ahead still in flight belongs to the state this call is about to void
  HIPCHK(hipMemcpyAsync(G->tok_dev, h, 4 * sizeof *h, hipMemcpyHostToDevice, G->main));
  gb25_status s = R->send_recv(m, G->tok_dev, G->tok_dev + 2, G->tok_dev + 4, G->tok_dev + 6, 2 * sizeof *h, G->main);
  if (s) return s;
  HIPCHK(hipMemcpyAsync(h + 4, G->tok_dev + 4, 4 * sizeof *h, hipMemcpyDeviceToHost, G->main));
  HIPCHK(hipStreamSynchronize(G->main));
  for (int q = 0; q < 2; q++)
    if (h[4 + 2 * q] != h[0] || h[5 + 2 * q] != h[1])
      return fail(m, GB25_ERR_STATE,
                  "collective call mismatch on rank %d: this rank made call %u(%u, %g) but its %s neighbour made call "
                  "%llu(%llu): setters of a decomposed model must be called alike on every rank",
                  R->rank, op, arg, payload, q == 0 ? "west" : "east", h[4 + 2 * q] >> 32, h[4 + 2 * q] & 0xffffffffull);
  return GB25_OK;
}

}  // namespace
