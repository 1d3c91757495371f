"""x-slab multi-GPU models: one process (rank) per GPU, packed halo exchange between ring neighbours.

Replaces what the reference gets from `Oceananigans.Distributed(arch; partition=Partition(Rx, Ry, 1))` + XLA's SPMD
partitioner (GB-25 sharding/sharded_baroclinic_instability_simulation_run.jl:65-72).  The sequencing of a slab's time
step, the pack / unpack kernels and the exchanges all live INSIDE the library (csrc/slab_step.hpp): after the exchange
context exists, `first_time_step`, `time_step` and `loop` are one ABI call each, exactly as on a single GPU.  This
module only

  * bootstraps the RCCL communicator: rank 0 asks the library for the 128-byte unique id (ncclGetUniqueId) and hands it
    to the other ranks through torch.distributed's rendezvous store (any broadcast would do: MPI in a Julia host);
  * offers the two other transports the library knows: all slabs in one process (`LocalSlabEnsemble`: decomposition
    invariance tests on a one-GPU box) and a host-side exchange through torch.distributed point-to-point operations
    (`TorchDistributedTransport`: rehearsal of the multi-process path with gloo where RCCL cannot run, e.g. two ranks
    on one device).
No collective is needed in a time step: every rank talks to its west and east neighbour only.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from .binding import GB25Error, HipBackend, StateMonitor
from .correctness import combine_diffs, combine_stats, _best   # noqa: F401  (combine_*: the host arithmetic over ranks)
from .model import HydrostaticFreeSurfaceModel
from .sharding import mesh_neighbours, slab_neighbours

WEST, EAST = 0, 1


class TorchDistributedTransport:
    """Ring exchange with torch.distributed point-to-point ops (the host-callback transport of the library).

    Posting order is part of the protocol: sends [west pack, east pack], receives [east halo, west halo].
    With two ranks both neighbours are the same peer and messages between one pair match in posting order,
    so the peer's FIRST send (its west pack) must meet our FIRST receive (our east halo)."""

    def __init__(self, rank, nranks, dist=None, ranks_y=1):
        import torch.distributed as tdist
        self.dist = dist or tdist
        self.rank, self.nranks = rank, nranks
        # Partition(Rx, Ry, 1): the ring runs within the rank's row; south / north are None beyond the walls
        nb = mesh_neighbours(rank, nranks // max(1, ranks_y), max(1, ranks_y))
        self.west, self.east, self.south, self.north, self.partner = (nb[k] for k in ("west", "east", "south", "north", "partner"))

    def exchange(self, send_west, send_east, recv_west, recv_east):
        d = self.dist
        stage = send_west.is_cuda and d.get_backend() != "nccl"
        if stage:
            # gloo has no device-memory point-to-point: bounce through host buffers
            dev = (recv_west, recv_east)
            send_west, send_east = send_west.cpu(), send_east.cpu()
            recv_west, recv_east = torch.empty_like(send_west), torch.empty_like(send_east)
        ops = [d.P2POp(d.isend, send_west, self.west), d.P2POp(d.isend, send_east, self.east),
               d.P2POp(d.irecv, recv_east, self.east), d.P2POp(d.irecv, recv_west, self.west)]
        for req in d.batch_isend_irecv(ops):
            req.wait()
        if stage:
            dev[0].copy_(recv_west)
            dev[1].copy_(recv_east)
            torch.cuda.current_stream().synchronize()     # the library's streams know nothing of torch's


    def exchange_partner(self, send, recv):
        """Zipper fold of a decomposed tripolar grid: slab r <-> slab P-1-r (buffer sets 3 and 4 of the library)."""
        d = self.dist
        partner = self.partner
        if partner == self.rank:
            recv.copy_(send)
            return
        stage = send.is_cuda and d.get_backend() != "nccl"
        dev = recv
        if stage:
            send, recv = send.cpu(), torch.empty_like(send, device="cpu")
        for req in d.batch_isend_irecv([d.P2POp(d.isend, send, partner), d.P2POp(d.irecv, recv, partner)]):
            req.wait()
        if stage:
            dev.copy_(recv)
            torch.cuda.current_stream().synchronize()


    def exchange_y(self, send_south, send_north, recv_south, recv_north):
        """y halos of a 2-D decomposition (buffer sets 5 - 7 of the library): my southern pack -> the southern neighbour's
        northern halo, my northern pack -> the northern neighbour's southern halo; None where there is no neighbour."""
        d = self.dist
        pairs = [(send_south, recv_south, self.south), (send_north, recv_north, self.north)]
        pairs = [(s_, r_, peer) for s_, r_, peer in pairs if peer is not None]
        if not pairs:
            return
        stage = pairs[0][0].is_cuda and d.get_backend() != "nccl"
        dev = [r_ for _, r_, _ in pairs]
        if stage:
            pairs = [(s_.cpu(), torch.empty_like(s_, device="cpu"), peer) for s_, _, peer in pairs]
        ops = [d.P2POp(d.isend, s_, peer) for s_, _, peer in pairs] + [d.P2POp(d.irecv, r_, peer) for _, r_, peer in reversed(pairs)]
        for req in d.batch_isend_irecv(ops):
            req.wait()
        if stage:
            for t, (_, r_, _) in zip(dev, pairs):
                t.copy_(r_)
            torch.cuda.current_stream().synchronize()


class _DevicePointer:
    """A device buffer of the library seen by torch (zero-copy) through __cuda_array_interface__."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def _as_tensor(ptr, nbytes, device):
    return torch.as_tensor(_DevicePointer(ptr, nbytes), device=device)


def share_unique_id(backend, rank, dist=None):
    """ncclGetUniqueId on rank 0, handed to every rank through torch.distributed (object broadcast: works with any
    backend).  A Julia host would MPI.Bcast the same 128 bytes."""
    import torch.distributed as tdist
    d = dist or tdist
    box = [backend.comm_unique_id() if rank == 0 else None]
    d.broadcast_object_list(box, src=0)
    return box[0]


class SlabModel(HydrostaticFreeSurfaceModel):
    """One rank's slab of a (Nx_global x Ny x Nz) model; same API as the single-GPU model: first_time_step / time_step
    / loop are ONE library call each.  Fields are the LOCAL slab (Nx_global / nranks columns).

    transport: "rccl" (default when torch.distributed runs on the nccl backend) -- the library's own communicator,
               ncclSend/ncclRecv on its second HIP stream;  "host" -- torch.distributed point-to-point through the
               library's callback transport (gloo rehearsal)."""

    def __init__(self, Nx_global, Ny, Nz, *, dt, rank, nranks, device=0, halo=8, substeps=30, transport=None, ranks_y=1, **kw):
        import torch.distributed as dist
        # ranks_y > 1: Partition(nranks / ranks_y, ranks_y, 1), rank = ry Rx + rx; the fields are the rank's window of columns
        # AND rows
        backend = HipBackend(Nx_global, Ny, Nz, dt=dt, halo=halo, substeps=substeps, device=device, rank=rank,
                             nranks=nranks, ranks_y=ranks_y, **kw)
        super().__init__(backend, backend.Nx_local, backend.Ny_local, Nz, halo)
        self.rank, self.nranks, self.ranks_y = rank, nranks, ranks_y
        if transport is None:
            transport = "rccl" if (nranks == 1 or os.environ.get("GB25_REHEARSE_ALONE") == "1" or dist.get_backend() == "nccl") else "host"
        self.transport_kind = transport
        if transport == "rccl":
            # (GB25_REHEARSE_ALONE=1: one rank of a decomposition alone in its process, its own neighbour on every side)
            alone = nranks == 1 or os.environ.get("GB25_REHEARSE_ALONE") == "1"
            uid = backend.comm_unique_id() if alone else share_unique_id(backend, rank)
            backend.comm_init_rccl(uid)
        elif transport == "host":
            self._ring = TorchDistributedTransport(rank, nranks, ranks_y=ranks_y)
            dev = torch.device("cuda", device)

            def exchange(buffer_set, sw, se, rw, re, nbytes):
                # whom a buffer set travels to (Peer in csrc/slab_protocol.hpp): 0 - 2, 8: the west / east ring neighbours;
                # 3, 4, 10: the fold partner; 5 - 7, 9: the southern / northern neighbour (8 - 10: CATKE's e and J^b)
                kind = 1 if buffer_set in (3, 4, 10) else 2 if buffer_set in (5, 6, 7, 9) else 0
                if kind == 2:            # y halos: (south, north) in the place of (west, east); null where there is no neighbour
                    t = lambda p: _as_tensor(p, nbytes, dev) if p else None
                    self._ring.exchange_y(t(sw), t(se), t(rw), t(re))
                    if torch.cuda.is_available():
                        torch.cuda.current_stream().synchronize()
                    return
                if kind == 1:            # to and from the fold partner (the east pointers are null)
                    self._ring.exchange_partner(_as_tensor(sw, nbytes, dev), _as_tensor(rw, nbytes, dev))
                    if torch.cuda.is_available():
                        torch.cuda.current_stream().synchronize()
                    return
                self._ring.exchange(_as_tensor(sw, nbytes, dev), _as_tensor(se, nbytes, dev),
                                    _as_tensor(rw, nbytes, dev), _as_tensor(re, nbytes, dev))
            backend.comm_init_callback(exchange)
        else:
            raise ValueError(f"transport must be 'rccl' or 'host', got {transport!r}")


class LocalSlabEnsemble:
    """P slabs of one global model stepped in lock-step inside ONE process on one GPU: the library's local transport
    (ring of device-to-device copies), the same stages, pack / unpack kernels and two streams as the RCCL path."""

    def __init__(self, Nx_global, Ny, Nz, P, *, dt, device=0, ranks_y=1, **kw):
        # ranks_y > 1: a 2-D decomposition, Partition(P / ranks_y, ranks_y, 1); rank = ry Rx + rx
        self.P, self.Ry, self.Rx = P, ranks_y, P // ranks_y
        self.Nx_loc, self.Ny_loc = Nx_global // self.Rx, Ny // ranks_y
        self.backends = [HipBackend(Nx_global, Ny, Nz, dt=dt, device=device, rank=r, nranks=P, ranks_y=ranks_y, **kw)
                         for r in range(P)]
        HipBackend.comm_init_local(self.backends)

    def scatter(self, name, global_interior):
        for b in self.backends:
            d = b.field_dims(name, False)      # (a y-face field has one row more on the ranks that hold the northern wall)
            i0, j0 = b.rx * self.Nx_loc, b.ry * self.Ny_loc
            b.set_field(name, np.ascontiguousarray(global_interior[i0:i0 + d[0], j0:j0 + d[1]]), False)

    def gather(self, name):
        rows = [np.concatenate([self.backends[ry * self.Rx + rx].get_field(name, False) for rx in range(self.Rx)], axis=0)
                for ry in range(self.Ry)]
        return rows[0] if self.Ry == 1 else np.concatenate(rows, axis=1)

    # diagnostics: every slab reduces its own interior on the device (local, not collective), the host combines
    def field_stats(self, name):
        return combine_stats([b.field_stats(name, False) for b in self.backends])

    def state_monitor(self):
        mons = [b.state_monitor() for b in self.backends]
        out = StateMonitor()
        for name in ("u", "v", "w", "eta", "T", "S"):
            setattr(out, name, combine_stats([getattr(m, name) for m in mons]))
        # (the CFL record has no offset of its own: the cells are the interior of u)
        cfls = [SimpleNamespace(cfl=m.cfl, at_cfl=m.at_cfl, global_offset=m.u.global_offset) for m in mons]
        out.cfl, at = _best(cfls, lambda r: r.cfl, "at_cfl")
        out.at_cfl[:] = at
        out.nonfinite_total = sum(m.nonfinite_total for m in mons)
        out.iteration, out.time = mons[0].iteration, mons[0].time
        return out

    # integrals: likewise (gb-25_amd/integrals.py)
    def integrate_field(self, name, shape="total"):
        from .integrals import combine_moments
        return combine_moments([b.integrate_field(name, shape) for b in self.backends], [b.ry * self.Ny_loc for b in self.backends])

    def budget(self):
        from .integrals import combine_budgets
        return combine_budgets([b.budget() for b in self.backends])

    # transports: likewise (gb-25_amd/transports.py); window = (first, count) of the GLOBAL summed index -- i for "across_y",
    # j for "across_x" --, clipped to every rank's interior; a rank the window misses is not asked
    def transport(self, faces, shape="lines", window=None):
        from .transports import _window, combine_transports
        y = faces == "across_y"
        w = _window(window, self.Nx_loc * self.Rx if y else self.Ny_loc * self.Ry)
        n = self.Nx_loc if y else self.Ny_loc
        parts, offsets = [], []
        for b in self.backends:
            i0, j0 = b.rx * self.Nx_loc, b.ry * self.Ny_loc
            at = i0 if y else j0
            lo, hi = max(w.start, at), min(w.stop, at + n)
            if lo < hi:
                parts.append(b.transport(faces, "lines", (lo - at, hi - lo)))
                offsets.append((i0, j0))
        return combine_transports(parts, faces, offsets, shape)

    # sums in classes: likewise (gb-25_amd/classes.py); window = (first, count) of the GLOBAL i, clipped to every rank's interior
    def class_sums(self, what, variable, edges, shape="rows", window=None):
        from .classes import combine_class_sums
        from .transports import _window
        w = _window(window, self.Nx_loc * self.Rx)
        parts, offsets = [], []
        for b in self.backends:
            i0, j0 = b.rx * self.Nx_loc, b.ry * self.Ny_loc
            lo, hi = max(w.start, i0), min(w.stop, i0 + self.Nx_loc)
            if lo < hi:
                parts.append(b.class_sums(what, variable, edges, "rows", (lo - i0, hi - lo)))
                offsets.append((i0, j0))
        return combine_class_sums(parts, what, offsets, shape)

    # zonal spectra: likewise (gb-25_amd/spectra.py); every slab transforms its own part of the lines with the global column and
    # N, the parts add.  nonfinite_lines counts the skipped lines of the ranks (a line is skipped by the ranks that hold the value)
    def zonal_spectrum(self, source, wavenumbers=None, levels=None, param=None):
        from .spectra import combine_spectra
        parts = [b.zonal_spectrum(source, wavenumbers, levels, param) for b in self.backends]
        offsets = [(b.rx * self.Nx_loc, b.ry * self.Ny_loc) for b in self.backends]
        return combine_spectra([p[0] for p in parts], offsets), sum(p[1] for p in parts)

    # fields on surfaces: every slab searches its own columns, the results are placed by global offset (gb-25_amd/surfaces.py)
    def on_surfaces(self, variable, carried, values):
        from .surfaces import gather_surfaces
        return gather_surfaces(self, variable, carried, values)

    # stability diagnostics: every slab computes its own columns, the results are placed by global offset (gb-25_amd/stability.py)
    def stability(self, kind, param=None, levels=None):
        from .stability import gather_stability
        return gather_stability(self, kind, param, levels)

    # flow kinematics: every slab computes its own interior from the halos the step left, placed by global offset (gb-25_amd/kinematics.py)
    def kinematics(self, kind, param=None, levels=None):
        from .kinematics import gather_kinematics
        return gather_kinematics(self, kind, param, levels)

    # zonal-mean and eddy statistics (gb-25_amd/eddies.py): two phases, so that the eddies are those about the GLOBAL mean of a line --
    # every slab reduces its part of the lines, the parts add in rank order and give the mean; every slab is asked again with the
    # mean of its rows, and the comoments add in rank order; rows are stacked in y on a mesh.  `measure` is summed over the whole
    # line in the order of ONE domain from the cells' static measure (gathered once per ensemble: forget_measure() after a setter
    # of the grid or of the bottom), so it does not depend on the decomposition
    def zonal_eddy(self, levels=None):
        from .eddies import ZonalEddy, combine_zonal_eddy, gathered_measure, single_domain_measure
        if getattr(self, "_cell_measure", None) is None:
            self._cell_measure = gathered_measure(self.backends)
        measure = single_domain_measure(self._cell_measure, self.backends[0].cfg.halo, levels)
        offsets = [b.ry * self.Ny_loc for b in self.backends]
        mean = combine_zonal_eddy([b.zonal_eddy(levels) for b in self.backends], offsets, measure)["mean"]
        parts = [b.zonal_eddy(levels, mean[o:o + self.Ny_loc]) for b, o in zip(self.backends, offsets)]
        return ZonalEddy(combine_zonal_eddy(parts, offsets, measure), levels)

    def forget_measure(self):
        self._cell_measure = None

    # block sums: every slab reduces its own blocks -- a block that does not divide a slab's extents is that slab's error --, the
    # planes are placed by global offset (gb-25_amd/blocks.py)
    def block_sums(self, source, block, levels=None, level_weights=None, param=None):
        from .blocks import block_sums, gather_blocks
        return gather_blocks([block_sums(b, source, block, levels, level_weights, param) for b in self.backends])

    # moving-window filter: a window reaches beyond a slab, so the device entry refuses on a rank; the source and the measure are
    # gathered and the definition is applied on the host (gb-25_amd/filters.py): the single domain's planes bit for bit
    def filter_sums(self, source, radius, stride=(1, 1), levels=None, wx=None, wy=None, rx_of_row=None):
        from .filters import ensemble_filter_sums
        return ensemble_filter_sums(self, source, radius, stride, levels, wx, wy, rx_of_row)

    # time averages: likewise (gb-25_amd/averages.py); every slab accumulates its own interior, the read-out is placed by
    # global offset
    def averages_begin(self, groups=("means", "squares", "fluxes"), levels=None):
        for b in self.backends:
            b.averages_begin(groups, levels)

    def averages_sample(self, weight=1.0):
        for b in self.backends:
            b.averages_accumulate(weight)

    def average(self, name, normalized=True):
        from .averages import gather_averages
        return gather_averages([b.get_average(name, normalized) for b in self.backends],
                               [(b.rx * self.Nx_loc, b.ry * self.Ny_loc) for b in self.backends])

    def averages_end(self):
        for b in self.backends:
            b.averages_end()

    # Lagrangian particles: every slab advances its own on the device; the hand-over of the particles that left a slab runs on
    # the host after each advance (gb-25_amd/particles.py exchange_particles).  Cells are GLOBAL here; x slabs and the 2-D mesh.
    def _offsets(self):
        return [(b.rx * self.Nx_loc, b.ry * self.Ny_loc) for b in self.backends]

    def _particles_put(self, parts):
        for b, p in zip(self.backends, parts):
            b.particles_set(p["i"], p["j"], p["k"], p["a"], p["b"], p["c"], 0)
        self._parts = parts

    def particles_begin(self, i, j, k, a=0.5, b=0.5, c=0.5):
        """Start particles in the GLOBAL cells (i, j, k); each goes to the slab that owns its cell."""
        from .particles import make_state
        s = make_state(i, j, k, a, b, c)
        s["id"] = np.arange(s["i"].size)
        parts = []
        for be, (i0, j0) in zip(self.backends, self._offsets()):
            own = (s["i"] >= i0) & (s["i"] < i0 + self.Nx_loc) & (s["j"] >= j0) & (s["j"] < j0 + self.Ny_loc)
            p = {q: x[own] for q, x in s.items()}
            p["i"], p["j"] = (p["i"] - i0).astype(np.int32), (p["j"] - j0).astype(np.int32)
            parts.append(p)
            be.particles_begin(s["i"].size)
        self._particles_put(parts)
        self.particles_moved = 0

    def particles_advance(self, dt, substeps=1):
        """Advance the particles of every slab over dt in `substeps` midpoint substeps and hand over those that left their slab
        after EVERY substep (a particle that has left waits for the hand-over, so a slab makes one substep per call; advance(dt, n)
        equals n calls of advance(dt / n, 1) bit for bit, which makes this the single domain's advance(dt, substeps)).  A slab
        that refuses (more than one cell per call) leaves every slab's particles where they were before the call."""
        from .particles import exchange_particles
        saved = self._parts
        for _ in range(int(substeps)):
            for b in self.backends:
                try:
                    b.particles_advance(float(dt) / float(int(substeps)), 1)
                except GB25Error:
                    self._particles_put(saved)     # (the slabs before it, and the substeps before this one, had moved theirs)
                    raise
            parts = []
            for b, old in zip(self.backends, self._parts):
                p = b.particles_get()
                p["id"] = old["id"]
                parts.append(p)
            parts, moved = exchange_particles(parts, self._offsets(), (self.Nx_loc, self.Ny_loc))
            self.particles_moved += moved
            if moved:
                self._particles_put(parts)
            else:
                self._parts = parts

    def _by_id(self, arrays):
        ids = np.concatenate([p["id"] for p in self._parts])
        out = np.concatenate(arrays)
        res = np.empty_like(out)
        res[ids] = out
        return res

    def particles_positions(self):
        """{"i", "j", "k" (GLOBAL cells), "a", "b", "c", "status", "rank"} in the order the particles were given."""
        Nx = self.Nx_loc * self.Rx
        out = {q: self._by_id([p[q] for p in self._parts]) for q in ("k", "a", "b", "c", "status")}
        out["i"] = self._by_id([(p["i"] + i0) % Nx for p, (i0, _) in zip(self._parts, self._offsets())]).astype(np.int32)
        out["j"] = self._by_id([p["j"] + j0 for p, (_, j0) in zip(self._parts, self._offsets())]).astype(np.int32)
        out["rank"] = self._by_id([np.full(p["i"].size, r) for r, p in enumerate(self._parts)])
        return out

    def particles_sample(self, name):
        return self._by_id([b.particles_sample(name) for b in self.backends])

    def particles_end(self):
        for b in self.backends:
            b.particles_end()

    def set_option(self, name, value):
        for b in self.backends:
            b.set_option(name, value)

    def synchronize(self):
        for b in self.backends:
            b.synchronize()

    # the composites of any member step every slab of the exchange context
    # checkpoint and restart: one file per rank, restart_rank<R>.gb25; a restore needs the same decomposition
    def checkpoint(self, directory, label="checkpoint", wait=True, max_arena_bytes=0):
        """Snapshot every rank (one launch each), then write the files -- or, with wait=False, return the handles whose write()
        does, while the ensemble steps on.  Returns the paths / the handles in rank order."""
        from .restart import Snapshot
        for b in self.backends:
            b.checkpoint_snapshot(max_arena_bytes)
        handles = [Snapshot(b, directory, label) for b in self.backends]
        return [h.write() for h in handles] if wait else handles

    def restore(self, directory, label="checkpoint"):
        """Every rank reads its own file (the exchange context exists from the ensemble's construction on); a refusal of one
        rank raises before the ranks behind it are touched.  Returns the RestoreInfo of every rank."""
        return [b.restore(directory, label) for b in self.backends]

    def first_time_step(self):
        self.backends[0].first_time_step()

    def time_step(self):
        self.backends[0].time_step()

    def loop(self, n):
        self.backends[0].loop(int(n))

    def close(self):
        for b in self.backends:
            b.close()
