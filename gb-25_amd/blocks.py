"""Block sums on the host: the definition of include/gb25.h ("block sums on the device") restated with numpy from a backend's
public getters alone -- get_field, get_derived, metric / metric2, bottom_info, field_dims -- in fp64 with the operation order of
the kernel (csrc/block_kernels.hpp, k_block_sums), so that the device's planes equal these bit for bit.  It is also what the
public functions fall back to on a backend without the kernel (the test suite's oracle backend).

    the interior is cut into boxes of bx x by x bz points; mu = integrals.cell_measure (THE MEASURE of gb25_integrate_field),
    mu' = mu * level_weights[k] (one multiply; none without weights); a point counts iff mu' > 0 and x is finite
    t = mu' * x,  q = t * x                                  (no fused multiply-add)
    c(i, j)  = the block's levels added in ascending k       (every sum starts from +0.0; what does not count adds nothing)
    s(I, j)  = c(i, j) over the block's bx columns, ascending i
    block    = s(I, j) over the block's by rows, ascending j
    measure = sum mu', first = sum t, second = sum q

Results are local to a rank: gather_blocks places the ranks' planes by their global offsets."""
import numpy as np

from .binding import DERIVED_IDS
from .integrals import cell_measure, location

PLANES = ("measure", "first", "second")
FLAT_OF = {"cc": "eta", "fc": "U", "cf": "V"}      # a 2-D field at each horizontal location: its measure is the column's area
MAX_BX = 256                                        # GB25_BLOCK_MAX_BX


class BlockSums:
    """The planes of one call, [I, J, K] float64 each (None: not asked for), and its info: dims, points and nonfinite totalled
    over the blocks, empty_blocks (measure 0), global_offset of the rank's FINE interior; block = (bx, by, bz).  points_of_blocks:
    the counted points per block (the host restatement alone fills it)."""

    def __init__(self, measure, first, second, *, block, dims, points, nonfinite, empty_blocks, global_offset=(0, 0, 0),
                 points_of_blocks=None):
        self.measure, self.first, self.second = measure, first, second
        self.block = tuple(int(q) for q in block)
        self.dims = tuple(int(q) for q in dims)
        self.points, self.nonfinite, self.empty_blocks = int(points), int(nonfinite), int(empty_blocks)
        self.global_offset = tuple(int(q) for q in global_offset)
        self.points_of_blocks = points_of_blocks

    @property
    def info(self):
        return dict(dims=self.dims, points=self.points, nonfinite=self.nonfinite, empty_blocks=self.empty_blocks,
                    global_offset=self.global_offset)

    def integral(self):
        """sum mu' x of every block: the integral of the field over the block's wet part."""
        return self.first

    def mean(self):
        """The measure-weighted mean of every block; NaN where the block has no counted point (measure 0)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.measure > 0, self.first / self.measure, np.nan)

    def variance(self):
        """second / measure - mean^2, clipped at 0: the variance below the block scale; NaN where measure is 0."""
        mean = self.mean()
        with np.errstate(invalid="ignore", divide="ignore"):
            v = self.second / self.measure - mean * mean
        return np.where(self.measure > 0, np.maximum(v, 0.0), np.nan)

    def __repr__(self):
        return f"BlockSums(block={self.block}, {', '.join(f'{k}={v}' for k, v in self.info.items())})"


def resolve(backend, source, block, levels=None, level_weights=None):
    """The checks of gb25_get_block_sums on the host: (measure name, fine extents (Nx, Ny, levels), k_first, k_count, dims,
    weights or None).  ValueError names the argument, as the library's message does."""
    derived = source in DERIVED_IDS
    if source == "vorticity":
        raise ValueError("source: the vorticity lives at (f,f,c), for which the measure is not defined")
    like = ("eta" if source == "mixed_layer_depth" else "T") if derived else source
    Nx, Ny, _ = backend.field_dims("T", False)
    nlev = backend.field_dims(like, False)[2]
    bx, by, bz = (int(q) for q in block)
    if bx <= 0 or bx > MAX_BX or Nx % bx:
        raise ValueError(f"bx = {bx} must be 1 .. {MAX_BX} and divide the rank's Nx = {Nx}")
    if by <= 0 or Ny % by:
        raise ValueError(f"by = {by} must be > 0 and divide the rank's Ny = {Ny}")
    k_first, k_count = (0, -1) if levels is None else (int(levels[0]), int(levels[1]))
    kc = nlev - k_first if k_count == -1 else k_count
    if k_first < 0 or k_first >= nlev or k_count < -1 or k_count == 0 or k_first + kc > nlev:
        raise ValueError(f"window k_first = {k_first}, k_count = {k_count} of {nlev} levels")
    if bz <= 0 or kc % bz:
        raise ValueError(f"bz = {bz} must be > 0 and divide the {kc} levels of the window")
    if level_weights is not None:
        if location(like)[1] is None:
            raise ValueError("level_weights must be None for a 2-D field")
        level_weights = np.ascontiguousarray(level_weights, np.float64).reshape(-1)
        if level_weights.size != nlev or not (np.isfinite(level_weights) & (level_weights >= 0)).all():
            raise ValueError(f"level_weights: {nlev} finite values >= 0, one per level of the field")
    return like, (Nx, Ny, nlev), k_first, kc, (Nx // bx, Ny // by, kc // bz), level_weights


def _global_offset(backend):
    return (int(getattr(backend, "rx", 0)) * int(getattr(backend, "Nx_local", 0)),
            int(getattr(backend, "ry", 0)) * int(getattr(backend, "Ny_local", 0)), 0)


def sums_of_blocks(x, mu, block, level_weights=None):
    """The definition on plain arrays: x [Nx, Ny, n] the values, mu [Nx, Ny, n] the measure, level_weights [n] or None, all of the
    window alone; Nx, Ny, n multiples of the block.  (measure, first, second, points, nonfinite), [I, J, K] each."""
    bx, by, bz = block
    x = np.asarray(x, np.float64)
    mu = np.asarray(mu, np.float64)
    if level_weights is not None:
        mu = mu * np.asarray(level_weights, np.float64)[None, None, :]
    nI, nJ, nK = x.shape[0] // bx, x.shape[1] // by, x.shape[2] // bz
    wet = mu > 0
    ok = wet & np.isfinite(x)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(ok, mu * np.where(ok, x, 0.0), 0.0)
        q = np.where(ok, t * np.where(ok, x, 0.0), 0.0)
    m = np.where(ok, mu, 0.0)
    out = []
    for a in (m, t, q):
        a = a.reshape(nI, bx, nJ, by, nK, bz)
        c = np.zeros(a.shape[:-1])
        for kk in range(bz):                  # the column partials, ascending k
            c = c + a[..., kk]
        s = np.zeros((nI, nJ, by, nK))
        for ii in range(bx):                  # the segments, ascending i
            s = s + c[:, ii]
        b = np.zeros((nI, nJ, nK))
        for jj in range(by):                  # the blocks, ascending j
            b = b + s[:, :, jj]
        out.append(b)
    shape6 = (nI, bx, nJ, by, nK, bz)
    points = ok.reshape(shape6).sum(axis=(1, 3, 5))
    nonfinite = (wet & ~ok).reshape(shape6).sum(axis=(1, 3, 5))
    return out[0], out[1], out[2], points, nonfinite


def block_sums_host(backend, source, block, levels=None, level_weights=None, *, param=None, values=None):
    """What HipBackend.block_sums returns, computed with numpy from the downloaded field (or derived field) and cell_measure: the
    restatement, bit for bit, and the fallback of a backend without the kernel.  source: a field name or a derived name at
    (c,c): "kinetic_energy", "density_anomaly", "potential_density", "mixed_layer_depth" (param: its threshold).  block = (bx, by,
    bz); levels = (k_first, k_count) of the field's own levels, None: all; level_weights: one per level of the field or None.
    values: the interior of the source, all its levels, where the backend cannot hand it out."""
    like, (Nx, Ny, nlev), k0, kc, dims, lw = resolve(backend, source, block, levels, level_weights)
    if values is not None:
        x = np.asarray(values)
    elif source in DERIVED_IDS:
        if hasattr(backend, "get_derived"):
            x = backend.get_derived(source, param)
        elif source == "kinetic_energy":
            from .derived import kinetic_energy_host
            x = kinetic_energy_host(backend)
        else:
            raise NotImplementedError(f"{source} needs a backend with get_derived, or values=")
    else:
        x = backend.get_field(source, False)
    x = np.asarray(x, np.float64)[:, :Ny, k0:k0 + kc]
    mu = cell_measure(backend, like)[:, :Ny, k0:k0 + kc]
    m, t, q, points, nonfinite = sums_of_blocks(x, mu, tuple(int(b) for b in block), None if lw is None else lw[k0:k0 + kc])
    return BlockSums(m, t, q, block=block, dims=dims, points=points.sum(), nonfinite=nonfinite.sum(), empty_blocks=(m == 0).sum(),
                     global_offset=_global_offset(backend), points_of_blocks=points)


def block_sums(backend, source, block, levels=None, level_weights=None, param=None):
    """From the device where the backend has the kernel, from the restatement where it has not."""
    if hasattr(backend, "block_sums"):
        return backend.block_sums(source, block, levels, level_weights, param)
    return block_sums_host(backend, source, block, levels, level_weights, param=param)


def depth_weights(backend, top, bottom, faces=False):
    """The fraction of every level that lies between the depths top <= bottom [m, positive], float64: [Nz] for the cells (level
    k spans the faces k and k + 1), [Nz + 1] with faces=True for the fields at (c,c,f) (level k spans the cell centres k - 1 and
    k, the first and the last end at the bottom and at the surface).  From metric("zf", .) in fp64; a level wholly inside the
    range gets exactly 1, one outside exactly 0."""
    top, bottom = float(top), float(bottom)
    if not 0.0 <= top <= bottom:
        raise ValueError(f"depth range: 0 <= top <= bottom, got ({top}, {bottom})")
    Nz = backend.field_dims("T", False)[2]
    zf = np.array([backend.metric("zf", k) for k in range(1, Nz + 2)], np.float64)
    edges = zf
    if faces:
        zc = 0.5 * (zf[:-1] + zf[1:])
        edges = np.concatenate([zf[:1], zc, zf[-1:]])
    deep, shallow = -edges[:-1], -edges[1:]            # the depths of a level's lower and upper end
    inside = np.minimum(bottom, deep) - np.maximum(top, shallow)
    thick = deep - shallow
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((inside > 0) & (thick > 0), inside / thick, 0.0)


def gather_blocks(parts):
    """One BlockSums from the ranks' (the same block, the same levels): every plane placed by the rank's global offset -- block
    (I, J) of a rank lies at (offset_x / bx + I, offset_y / by + J) --, the counts added, the smallest offset kept."""
    parts = list(parts)
    bx, by, _ = parts[0].block
    for p in parts:
        if p.block != parts[0].block or p.global_offset[0] % bx or p.global_offset[1] % by:
            raise ValueError("gather_blocks: the parts' blocks differ, or a rank's offset is no multiple of the block")
    at = [(p.global_offset[0] // bx, p.global_offset[1] // by) for p in parts]
    nI = max(a[0] + p.dims[0] for a, p in zip(at, parts))
    nJ = max(a[1] + p.dims[1] for a, p in zip(at, parts))
    nK = parts[0].dims[2]
    planes = {}
    for name in PLANES + ("points_of_blocks",):
        if any(getattr(p, name) is None for p in parts):
            planes[name] = None
            continue
        out = np.zeros((nI, nJ, nK), getattr(parts[0], name).dtype)
        for (I0, J0), p in zip(at, parts):
            out[I0:I0 + p.dims[0], J0:J0 + p.dims[1]] = getattr(p, name)
        planes[name] = out
    return BlockSums(planes["measure"], planes["first"], planes["second"], block=parts[0].block, dims=(nI, nJ, nK),
                     points=sum(p.points for p in parts), nonfinite=sum(p.nonfinite for p in parts),
                     empty_blocks=sum(p.empty_blocks for p in parts),
                     global_offset=tuple(min(p.global_offset[q] for p in parts) for q in range(3)),
                     points_of_blocks=planes["points_of_blocks"])


def column_area(backend, source):
    """The area of every column of the source's horizontal location [i, j] (1/2 on the pivot row, 0 over land): the measure of
    a 2-D field of that location, block (1, 1, 1)."""
    like = "T" if source in DERIVED_IDS else source
    return block_sums(backend, FLAT_OF[location(like)[0]], (1, 1, 1)).measure[:, :, 0]


def column_sums(backend, source, depth_range=None, param=None):
    """The block sums of whole columns, block (1, 1, levels), weighted with depth_weights where depth_range = (top, bottom) is
    given.  A 2-D source (the mixed-layer depth) is one level."""
    like = ("eta" if source == "mixed_layer_depth" else "T") if source in DERIVED_IDS else source
    nlev = backend.field_dims(like, False)[2]
    lw = None
    if depth_range is not None:
        lw = depth_weights(backend, depth_range[0], depth_range[1], faces=location(like)[1] == "f")
    return block_sums(backend, source, (1, 1, nlev), None, lw, param)
