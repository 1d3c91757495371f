// slab_protocol.hpp -- the vocabulary of the decomposed step (slab_step.hpp): its stages, exchange groups, buffer sets, streams, event
// slots and local operations, and ONE table that says what a group is.  Plain C++, no HIP.  The numbers are fixed: the dry runs print
// them (gb25_debug_sequence, gb25_debug_exchange_plan; tests/test_distributed_cpu.py parses them) and the buffer set numbers are ABI
// (gb25_exchange_fn, include/gb25.h; gb-25_amd/distributed.py).  The table with what travels and when: DESIGN.md, "The exchange groups
// of a decomposed step".
#pragma once
namespace {

// What one slab does between exchanges (slab_stage).  The sequencer picks the sub-case; no stage function looks at the number.
enum Stage : int {
  Update = 0,                   // AB2 update, adoption of the look-aheads, y/z layers of the bundle, own columns' pressure forked
  Subcycle = 1,                 // this step's sub-cycle (fold / 2-D decomposition: only the interior copy into the work arrays)
  SubcycleAhead = 5,            // ... the NEXT step's, beside the tracer tendencies
  SubcycleSubsteps = 16,        // fold / 2-D decomposition: the substeps, once the rows of the work arrays have travelled
  SubcycleAheadSubsteps = 56,
  OwnColumns = 2,               // corrector on the own columns, their y/z layers and w, interior momentum tendencies
  LazyHead = 20,                // a lazy step: du, dv and the chunk bases of w only, ahead of the wait for the packed bundle
  StripsOnComm = 33,            // the two pressure strips next to the x halos, on the exchange stream behind the unpacked bundle
  HaloRowsCorrector = 32,       // 2-D decomposition: corrector on the x halo columns of the own rows, before the rows leave
  HaloColumns = 3,              // corrector in the halo columns, fills, w, pressure strips, edge momentum tendencies
  HaloColumnsToLayers = 30,     // fold: ... up to the y/z layers (then the rows beyond the fold arrive)
  HaloColumnsRest = 31,         // fold: ... the rest
  Tracers = 4,                  // tracer tendencies (CATKE: and the step of e on the own columns)
  CatkeFinish = 41,             // CATKE: diffusivities and the slow tendency of e, once the halos of e and J^b are in
};

// What travels in one exchange.  (`Ahead`: the same pieces for the sub-cycle look-ahead -- G.U, G.V come from the momentum
// look-ahead's partner buffers.)
enum Group : int {
  Bundle = 0,                   // H columns of u, v, T, S and the column integrals of u, v
  BaroWide = 1,                 // W columns of eta, U, V, G.U, G.V -> the wide halos of the sub-cycle's work arrays
  BaroHalo = 2,                 // H columns of eta, U, V (the initial state)
  BaroWideAhead = 3,
  BaroHaloAhead = 4,            // (unused: the widened sub-cycle leaves the x halo columns of the new eta, U, V behind)
  FoldBundle = 6,               // the H rows south of the pivot row of u, v, T, S, eta, U, V -> the fold partner
  FoldTall = 8,                 // the Wy (+1) rows south of the pivot row of the sub-cycle's work arrays -> the fold partner
  BundleRows = 10,              // 2-D decomposition: H rows of u, v, T, S (and the column integrals of a lazy step)
  BaroWideRows = 11,            // ... W rows of the sub-cycle's work arrays, all widened columns
  BaroHaloRows = 12,            // ... H rows of eta, U, V (the initial state)
  BaroWideRowsAhead = 13,
  BaroHaloRowsAhead = 14,       // (unused, as BaroHaloAhead)
  CatkeColumns = 20,            // closure = CATKE: H columns of e and J^b after the step of e
  CatkeRows = 21,               // ... their H rows
  CatkeFold = 22,               // ... their H rows south of the pivot row
};

// A buffer set: one send and one receive buffer per side and slab.  Groups that never overlap in time share a set.
enum BufferSet : int {
  SetBundle = 0, SetBaroWide = 1, SetBaroHalo = 2, SetFoldBundle = 3, SetFoldTall = 4, SetBundleRows = 5, SetBaroWideRows = 6,
  SetBaroHaloRows = 7, SetCatkeColumns = 8, SetCatkeRows = 9, SetCatkeFold = 10,
  NSETS
};

// Whom a buffer set travels to: the west / east neighbours of the ring (sides 0 / 1), the fold partner (side 0 only), the southern /
// northern neighbour of a 2-D decomposition (sides 0 / 1, where they exist).
enum class Peer { Ring, FoldPartner, Rows };
// Which kernel packs and unpacks a group: k_move_columns, k_move_rows, k_fold_pack / k_fold_unpack, k_tall_rows.
enum class Mover { Columns, Rows, FoldRows, TallRows };

struct GroupInfo {
  Group group;
  BufferSet set;
  Peer peer;
  Mover mover;
  bool closure;   // the closure's fields (e, J^b) instead of the model's
};
constexpr GroupInfo kGroups[] = {
    {Group::Bundle,            SetBundle,       Peer::Ring,        Mover::Columns,  false},
    {Group::BaroWide,          SetBaroWide,     Peer::Ring,        Mover::Columns,  false},
    {Group::BaroHalo,          SetBaroHalo,     Peer::Ring,        Mover::Columns,  false},
    {Group::BaroWideAhead,     SetBaroWide,     Peer::Ring,        Mover::Columns,  false},
    {Group::BaroHaloAhead,     SetBaroHalo,     Peer::Ring,        Mover::Columns,  false},   // unused
    {Group::FoldBundle,        SetFoldBundle,   Peer::FoldPartner, Mover::FoldRows, false},
    {Group::FoldTall,          SetFoldTall,     Peer::FoldPartner, Mover::TallRows, false},
    {Group::BundleRows,        SetBundleRows,   Peer::Rows,        Mover::Rows,     false},
    {Group::BaroWideRows,      SetBaroWideRows, Peer::Rows,        Mover::Rows,     false},
    {Group::BaroHaloRows,      SetBaroHaloRows, Peer::Rows,        Mover::Rows,     false},
    {Group::BaroWideRowsAhead, SetBaroWideRows, Peer::Rows,        Mover::Rows,     false},
    {Group::BaroHaloRowsAhead, SetBaroHaloRows, Peer::Rows,        Mover::Rows,     false},   // unused
    {Group::CatkeColumns,      SetCatkeColumns, Peer::Ring,        Mover::Columns,  true},
    {Group::CatkeRows,         SetCatkeRows,    Peer::Rows,        Mover::Rows,     true},
    {Group::CatkeFold,         SetCatkeFold,    Peer::FoldPartner, Mover::FoldRows, true},
};
// (a number from outside the library -- gb25_debug_exchange_plan -- may name no group: null)
constexpr const GroupInfo* find_group(int group) {
  for (const GroupInfo& r : kGroups)
    if (r.group == group) return &r;
  return nullptr;
}
constexpr const GroupInfo& group_info(Group group) { return *find_group(group); }
// The first group of a set: the one its buffers are sized for (the others of the set carry pieces of the same sizes).
constexpr const GroupInfo& set_info(BufferSet b) {
  for (const GroupInfo& r : kGroups)
    if (r.set == b) return r;
  return kGroups[0];
}
constexpr int set_sides(BufferSet b) { return set_info(b).peer == Peer::FoldPartner ? 1 : 2; }

// What the arithmetic on group and set numbers used to encode:
constexpr bool every_set_has_one_peer_and_mover() {
  for (int b = 0; b < NSETS; b++) {
    int rows = 0;
    for (const GroupInfo& r : kGroups) {
      if (r.set != b) continue;
      rows++;
      if (r.peer != set_info((BufferSet)b).peer || r.mover != set_info((BufferSet)b).mover) return false;
    }
    if (rows == 0) return false;
  }
  return true;
}
constexpr bool movers_fit_peers() {   // columns go round the ring, rows to the southern / northern neighbour, the rest to the fold partner
  for (const GroupInfo& r : kGroups) {
    const Peer want = r.mover == Mover::Columns ? Peer::Ring : r.mover == Mover::Rows ? Peer::Rows : Peer::FoldPartner;
    if (r.peer != want) return false;
  }
  return true;
}
constexpr bool groups_ascend() {
  for (unsigned i = 1; i < sizeof kGroups / sizeof *kGroups; i++)
    if (kGroups[i - 1].group >= kGroups[i].group) return false;
  return true;
}
static_assert(every_set_has_one_peer_and_mover(), "every buffer set 0 .. NSETS-1 has groups, and they agree on the peer and the mover");
static_assert(movers_fit_peers(), "the mover of a group fits whom it travels to");
static_assert(groups_ascend(), "one row per group");
static_assert(set_sides(SetFoldBundle) == 1 && set_sides(SetFoldTall) == 1 && set_sides(SetCatkeFold) == 1 && set_sides(SetBundle) == 2,
              "a set that goes to the fold partner has one side, every other set two");
static_assert(NSETS == 11 && group_info(Group::CatkeFold).set == SetCatkeFold, "buffer set numbers are ABI (include/gb25.h)");

// The streams of a SlabGroup.  Sub: the substeps of the sub-cycle look-ahead, so that the next step's bundle -- posted on Comm right
// behind stage Update -- does not queue behind five sub-cycle launches it has nothing to do with.
enum StreamId : int { Main = 0, Comm = 1, Sub = 2 };
constexpr const char* kStreamNames[] = {"main", "comm", "sub"};

// What each event of a SlabGroup marks once recorded.
enum EventSlot : int {
  UpdateWritten = 0,        // everything stage Update wrote (Main)
  BundlePacked = 1,         // the bundle is packed: the corrector may rewrite the columns it was packed from (Comm)
  NextTendenciesExist = 2,  // the next step's G.U, G.V exist: the look-ahead chain may start (Main)
  HaloColumnsArrived = 3,   // everything on the exchange stream so far, the bundle's halo columns above all (Comm)
  ChainEnd = 4,             // the end of the look-ahead chain (Sub)
  ChainExchanged = 5,       // the chain's exchanges are unpacked: its substeps may start (Comm)
  NSLOTS
};

// What a slab does on its own inside first_time_step!, with the names the dry run prints.
enum LocalOp : int {
  Initialize = 0,
  FillLocal = 1,                    // y/z halo layers
  UpdateStateLocal = 2,             // update_state! without the x-halo fill
  MaskFillLocal = 3,                // fold: mask, y/z layers over the extended columns ...
  AuxiliariesTendenciesLocal = 4,   // ... and, once the rows beyond the fold are in, w, pressure, tendencies
  FirstFluxesLocal = 5,             // coupled model, iteration 0: the atmosphere-ocean fluxes of the initial state
  TendenciesLocal = 6,              // ... and the tendencies that see them
  CatkeFinishLocal = 7,             // CATKE: what stage CatkeFinish does inside a time step
};
constexpr const char* kLocalOpNames[] = {"initialize", "fill_local", "update_state_local", "mask_fill_local",
                                                 "auxiliaries_tendencies_local", "first_fluxes_local", "tendencies_local",
                                                 "catke_finish_local"};
static_assert(sizeof kLocalOpNames / sizeof *kLocalOpNames == CatkeFinishLocal + 1, "one name per local operation");

}  // namespace
