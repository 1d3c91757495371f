// diagnostics_state.hpp -- every piece of memory and bookkeeping the read-only diagnostics own (diagnostics_host.hpp,
// averages_host.hpp, classes_host.hpp, particles_host.hpp, spectrum_host.hpp, surfaces_host.hpp, stability_host.hpp, kinematics_host.hpp, region_host.hpp, zonal_eddy_host.hpp, blocks_host.hpp, filters_host.hpp), as ONE member of gb25_model.
// Host only; included by gb25_api.hip behind the kernel headers (PartState: particle_kernels.hpp; SURF_MAX: surface_kernels.hpp;
// GB25_A_COUNT and the info structs: include/gb25.h); like Field it is local to that translation unit, so the libraries export
// nothing of it.
// No stepping kernel reads or writes anything here.  release() is the one place that frees it (gb25_destroy), its two parts
// serve gb25_averages_end and gb25_particles_end; invalidate_tables() is what a rebuild of the grid or of the bottom calls.
#pragma once
#include <cstring>
#include <vector>

namespace {

// The results of ONE call of a family whose results grow with what the caller asks for: one allocation, made by the first call,
// made anew (nothing is kept) when a call needs more bytes than it holds.  A call never has less room than it asked for, and it
// finds its parts at offsets it computes from its OWN arguments, whatever else the buffer has room for.  grow() refuses before
// hipMalloc what the device has no room for (diag_room_for) and reports a failed hipMalloc as GB25_ERR_OUT_OF_MEMORY with the
// runtime's sticky error cleared; after either the buffer holds nothing.  (Defined in diagnostics_host.hpp: it reports through
// fail.)  The members of DiagState of this type are "a result buffer" below.
struct DiagBuffer {
  void* p = nullptr;
  size_t bytes = 0;
  void drop() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  gb25_status grow(gb25_model* m, const char* what, const char* of, size_t need);
};

struct DiagState {
  // field statistics (gb25_get_field_stats, gb25_compare_field, gb25_get_state_monitor): the per-block records of the reduction
  // kernels and the seven result records of a state monitor, one allocation made by the first call that needs it
  void* scratch = nullptr;
  size_t scratch_records = 0;
  // integrals (gb25_integrate_field, gb25_get_budget): the row, level and total records of up to five fields, made by the first
  // call that needs them
  void* moments = nullptr;
  size_t moments_rows = 0, moments_levels = 0;
  // diagnostics' own tables, made by the first call that needs them (moments_tables), dropped whenever the grid or the bottom
  // is rebuilt: by horizontal location the areas (curvilinear grids) and the first wet levels (grids with a bottom table); the
  // derived fields' AZFF (curvilinear grids) and (double) zc | zf; the transports' DXCF and DYFC (curvilinear grids); the
  // stability diagnostics' Coriolis parameter at (f,f) (curvilinear grids) and the first wet levels of the (c,c) columns WITH
  // the ring of columns around the interior (grids with a bottom table)
  gb25::real* area[3] = {nullptr, nullptr, nullptr};
  unsigned short* first_wet[3] = {nullptr, nullptr, nullptr};
  unsigned short* first_wet_ring = nullptr;
  gb25::real* azff = nullptr;
  gb25::real* fff = nullptr;
  double* zt = nullptr;
  gb25::real* face_length[2] = {nullptr, nullptr};
  bool tables_valid = false;
  // derived fields (gb25_compute_derived, gb25_get_field_levels): the packed result array -- one 2-D plane (the mixed-layer depth)
  // followed by room for the largest interior a field of this model has --, made by the first call that needs it; the TEOS-10
  // table folded at Z = 0 is part of the allocation of build_eos_tables, rebuilt with it and NOT freed here
  // (flow kinematics, gb25_compute_kinematics: their packed result lies in the 3-D part of the same array)
  gb25::real* derived = nullptr;
  size_t derived_plane = 0, derived_elems = 0;
  const double* eos0 = nullptr;
  // transports (gb25_get_transport): the LINES, running sums and PROFILE records of one call, made by the first call
  void* transport = nullptr;
  size_t transport_lines = 0;
  // class sums (gb25_get_class_sums): a result buffer -- the padded edges, then the ROWS, CUMULATIVE and TOTAL records of one call
  DiagBuffer class_sums;
  // zonal spectra (gb25_get_zonal_spectrum, gb25_get_derived_zonal_spectrum): a result buffer -- the count of skipped lines, then
  // the coefficients of one call.  The host word that count is copied into.  The interleaved copy of the table of the definition
  // on the device (one of diagnostics' own tables: dropped with them, made anew after a rebuild of the grid); k_zonal_spectrum's
  // dynamic-LDS attribute (only the instance with the table in LDS can pass 64 KB), per model as the others
  DiagBuffer spectrum;
  unsigned spec_skipped = 0;
  double* spec_table = nullptr;
  bool spec_valid = false, spec_lds_raised = false;
  // fields on surfaces (gb25_compute_on_surfaces, gb25_get_on_surfaces): a result buffer -- the padded targets (SURF_MAX
  // doubles), then the values and the status bytes of one call.  The host copy of the padded targets the upload reads (a word of
  // the model: no copy is ever pending from a frame that has returned)
  DiagBuffer surfaces;
  double surf_targets[gb25::SURF_MAX] = {};
  // stability diagnostics (gb25_compute_stability, gb25_get_stability): the packed result array, room for Nx x Ny x (Nz + 1)
  // values, made by the first call (ONE size per model, nothing grows: no result buffer)
  gb25::real* stability = nullptr;
  // zonal-mean and eddy statistics (gb25_get_zonal_eddy): a result buffer -- the line records of one call, then the caller's means
  DiagBuffer zonal_eddy;
  // block sums (gb25_get_block_sums, gb25_compute_block_sums, gb25_get_derived_block_sums): a result buffer -- the three counts of
  // the info record (BlockCounts, padded to 32 bytes), the level weights (Nz + 1 doubles), the planes measure | first | second
  // of one call, then the count slots of the waves of its launch.  The host copy of the weights the upload reads (a word of the
  // model: no copy is ever pending from a frame that has returned)
  DiagBuffer blocks;
  std::vector<double> block_weights;
  // moving-window filter (gb25_get_filter_sums, gb25_compute_filter_sums, gb25_get_derived_filter_sums): a result buffer -- the
  // counts of the info record (BlockCounts, padded to 32 bytes), the weights wx and wy (2 x 65 doubles), the radius of every row
  // (Ny int32), the planes measure | first | second of one call, the x pass's scratch planes, then the count slots of the waves
  // of its two launches.  The host copies the uploads read (words of the model: no copy is ever pending from a frame that has
  // returned)
  DiagBuffer filters;
  std::vector<double> filter_wx, filter_wy;
  std::vector<int32_t> filter_rows;
  // coherent regions (gb25_label_regions, gb25_get_regions): a result buffer -- the counts of the levels of one call, its label
  // planes, its records, then the scratch of ONE level: the union-find forest, the numbers at the keys, the blocks' root counts
  DiagBuffer regions;
  // time averages (gb25_averages_*): the accumulators of the active groups and the array a normalized read-out is divided into
  // -- ONE allocation (avg_acc[0] is its base: MEANS is always active), made by gb25_averages_begin, freed by gb25_averages_end
  // and gb25_destroy --, the window, the sample count and weight_sum (avg_info)
  double* avg_acc[GB25_A_COUNT] = {};
  double* avg_out = nullptr;
  gb25_averages_info avg_info = {};
  bool avg_on = false;
  // Lagrangian particles (gb25_particles_*): ONE allocation made by gb25_particles_begin, freed by gb25_particles_end and
  // gb25_destroy -- two copies of the state (an advance reads part_state[part_cur] and writes the other), the sample array, the
  // per-wave counter slots and their totals, the kbot table of every column the parents hold (made anew when the bottom is
  // rebuilt: part_tables_valid)
  void* part_base = nullptr;
  gb25::PartState part_state[2] = {};
  int part_cur = 0;
  double* part_sample = nullptr;
  unsigned* part_slots = nullptr;
  unsigned long long* part_totals = nullptr;
  int* part_kbot = nullptr;
  bool part_on = false, part_tables_valid = false;
  gb25_particles_info part_info = {};

  // the grid or the bottom was rebuilt: the next call that needs a table makes it anew
  void invalidate_tables() { tables_valid = part_tables_valid = spec_valid = false; }

  template <class T>
  static void drop(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  void release_tables() {
    for (auto& p : area) drop(p);
    for (auto& p : first_wet) drop(p);
    for (auto& p : face_length) drop(p);
    drop(first_wet_ring);
    drop(azff);
    drop(fff);
    drop(zt);
    drop(spec_table);
    tables_valid = spec_valid = false;
  }
  void release_averages() {
    drop(avg_acc[0]);   // (one allocation: the accumulators, then the read-out array)
    for (auto& p : avg_acc) p = nullptr;
    avg_out = nullptr;
    avg_on = false;
    memset(&avg_info, 0, sizeof avg_info);
  }
  void release_particles() {
    drop(part_base);   // (one allocation: every pointer below points into it)
    for (auto& s : part_state) s = {};
    part_sample = nullptr;
    part_slots = nullptr;
    part_totals = nullptr;
    part_kbot = nullptr;
    part_cur = 0;
    part_on = part_tables_valid = false;
    memset(&part_info, 0, sizeof part_info);
  }
  void release() {
    drop(scratch);
    drop(moments);
    drop(derived);
    drop(transport);
    drop(stability);
    for (DiagBuffer* b : {&class_sums, &spectrum, &surfaces, &zonal_eddy, &blocks, &filters, &regions}) b->drop();
    release_tables();
    release_averages();
    release_particles();
  }
};

}  // namespace
