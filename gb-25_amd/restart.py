"""Checkpoint and bit-for-bit restart (include/gb25.h, "checkpoint and bit-for-bit restart"; DESIGN.md, "Checkpoint and restart").

    handle = checkpoint(model, "run1", wait=False)   # one launch on the device; the drain runs beside what follows
    loop(model, 100)
    handle.write()                                   # waits for the drain only, writes run1/checkpoint/restart_rank0.gb25
    ...
    restore(fresh_model, "run1")                     # same configuration, grid and bottom set as in the run that wrote it

and the reader of the file for a host that wants the numbers: read_checkpoint, checksums, verify."""
import os
import struct

import numpy as np

MAGIC = b"GB25RST\x00"
VERSION = 1
HEADER = struct.Struct("<8s4I4QQ")        # magic, version, real_bytes, members, scalar_bytes, scalars/table/data offsets, file_bytes, reserved
ROW = struct.Struct("<48s6i5Q16x")        # name, field, extra, dims[3], elem_bytes, offset, bytes, arena_offset, s1, s2
CLOCK = struct.Struct("<ddq")             # the scalar block begins with time, last_dt, iteration
MAX_MEMBERS = 4096


class CheckpointError(ValueError):
    pass


def _need(backend, method):
    if not hasattr(backend, method):
        raise NotImplementedError("Checkpoint and restart need the HIP backend: this backend has no device snapshot kernel.")
    return getattr(backend, method)


class Snapshot:
    """What checkpoint(..., wait=False) returns: write() finishes the checkpoint, release() drops it."""

    def __init__(self, backend, directory, label):
        self.backend, self.directory, self.label, self.path = backend, directory, label, None

    def info(self):
        return self.backend.checkpoint_info()

    def write(self):
        if self.path is None:
            self.path = self.backend.checkpoint_write(self.directory, self.label)
        return self.path

    def release(self):
        """Drop the snapshot unwritten (and free the arena and the pinned buffers): the model may be snapshot again."""
        if self.path is None:
            self.backend.checkpoint_release()
            self.path = ""


def checkpoint(model, directory, label="checkpoint", wait=True, max_arena_bytes=0):
    """Snapshot the model's restart set on the device (one launch; the model may step on at once).  wait=True: also write
    <directory>/<label>/restart_rank<R>.gb25 and return its path; wait=False: return the Snapshot whose write() does."""
    b = model.backend
    _need(b, "checkpoint_snapshot")(max_arena_bytes)
    snap = Snapshot(b, directory, label)
    return snap.write() if wait else snap


def restore(model, directory, label="checkpoint"):
    """Fields, clock, scalar state and result-changing options of a checkpoint into `model`, which was created with the same
    configuration and given the same grid, bottom and atmosphere.  A refusal raises GB25Error naming what differs and leaves the
    model untouched.  Returns the RestoreInfo."""
    return _need(model.backend, "restore")(directory, label)


def run_checkpointed(model, steps, every, directory, label="checkpoint"):
    """loop(model, every), snapshot, and go on stepping while the snapshot drains; the file of a snapshot is written once the NEXT
    stretch of steps is in the queue.  Labels: <label>_<iteration>.  Returns the paths written."""
    b = model.backend
    _need(b, "checkpoint_snapshot")
    paths, pending, done = [], None, 0
    while done < steps:
        n = min(int(every), steps - done)
        b.loop(n)
        done += n
        if pending is not None:
            paths.append(pending.write())
        b.checkpoint_snapshot(0)
        pending = Snapshot(b, directory, f"{label}_{b.clock()[1]}")
    if pending is not None:
        paths.append(pending.write())
    return paths


# ---- the file ---------------------------------------------------------------------------------------------------------------
def checksums(array):
    """(s1, s2) of restart_file.hpp: s1 = sum x_n, s2 = sum (n + 1) x_n mod 2^64 over the bit patterns x_n of the elements (unsigned
    integers of their own width), n the 0-based index in memory order ([i, j, k] arrays: i fastest, Fortran order)."""
    a = np.asarray(array)
    if a.dtype.itemsize not in (4, 8):
        raise CheckpointError("checksums are defined for 4- and 8-byte elements")
    flat = np.ravel(a, order="F" if a.ndim > 1 else "C")
    x = flat.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)
    with np.errstate(over="ignore"):
        n1 = np.arange(1, x.size + 1, dtype=np.uint64)
        s1 = np.add.reduce(x, dtype=np.uint64) if x.size else np.uint64(0)
        s2 = np.add.reduce(n1 * x, dtype=np.uint64) if x.size else np.uint64(0)
    return int(s1), int(s2)


class Checkpoint:
    """header, clock (time, last_dt, iteration), the raw scalar block, and the members: {name: array [i, j, k]} memory-mapped,
    with `table[name]` = dict(field, extra, dims, offset, bytes, s1, s2)."""

    def __init__(self, path, real_bytes, clock, scalars, members, table):
        self.path, self.real_bytes, self.scalars, self.members, self.table = path, real_bytes, scalars, members, table
        self.time, self.last_dt, self.iteration = clock

    def __getitem__(self, name):
        return self.members[name]

    def names(self):
        return list(self.members)


def read_checkpoint(path):
    """Memory-map a checkpoint file.  Nothing of the table is believed before it is checked against the size of the file."""
    path = str(path)
    if path.endswith(".tmp"):
        raise CheckpointError(f"{path}: an unfinished checkpoint (*.tmp) is no checkpoint")
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        raw = f.read(HEADER.size)
        if len(raw) < HEADER.size:
            raise CheckpointError(f"{path}: shorter than a header")
        magic, version, real_bytes, members, scalar_bytes, scalars_off, table_off, data_off, file_bytes, _ = HEADER.unpack(raw)
        if magic != MAGIC:
            raise CheckpointError(f"{path}: not a gb25 checkpoint (magic)")
        if version != VERSION:
            raise CheckpointError(f"{path}: format version {version}, this reader knows {VERSION}")
        if real_bytes not in (4, 8):
            raise CheckpointError(f"{path}: real_bytes is neither 4 nor 8")
        if not 0 < members <= MAX_MEMBERS:
            raise CheckpointError(f"{path}: member count {members} out of bounds")
        if file_bytes != size:
            raise CheckpointError(f"{path}: truncated ({size} bytes of {file_bytes})")
        if scalars_off + scalar_bytes > size or scalar_bytes < CLOCK.size:
            raise CheckpointError(f"{path}: the scalar block lies beyond the end of the file")
        if table_off + members * ROW.size > size:
            raise CheckpointError(f"{path}: the member table lies beyond the end of the file")
        f.seek(scalars_off)
        scalars = f.read(scalar_bytes)
        f.seek(table_off)
        rows = f.read(members * ROW.size)
    out, table = {}, {}
    for q in range(members):
        name, field, extra, nx, ny, nz, eb, off, nbytes, _arena, s1, s2 = ROW.unpack_from(rows, q * ROW.size)
        name = name.split(b"\0")[0].decode()
        if off < data_off or off + nbytes > size:
            raise CheckpointError(f"{path}: member {name} lies beyond the end of the file")
        if eb not in (4, 8) or min(nx, ny, nz) < 0 or nx * ny * nz * eb != nbytes:
            raise CheckpointError(f"{path}: member {name} states dims that are not its bytes")
        dtype = np.float32 if eb == 4 else np.float64
        out[name] = np.memmap(path, dtype=dtype, mode="r", offset=off, shape=(nx, ny, nz), order="F")
        table[name] = dict(field=field, extra=extra, dims=(nx, ny, nz), offset=off, bytes=nbytes, s1=s1, s2=s2)
    return Checkpoint(path, real_bytes, CLOCK.unpack_from(scalars), scalars, out, table)


def verify(path):
    """Read every member and compare its checksums with the table's; returns the names that differ (empty: the file is sound)."""
    c = read_checkpoint(path)
    return [n for n, a in c.members.items() if checksums(a) != (c.table[n]["s1"], c.table[n]["s2"])]
