"""compare_states / sync_states! of the reference (GB-25 src/correctness.jl:4-103).

`isapprox(a, b; rtol, atol)` on Julia arrays is a NORM test:
    norm(a - b) <= max(atol, rtol * max(norm(a), norm(b)))
and that is what `approx_equal` implements.  The report line has the same content as the
reference's @printf (name, verdict, max|psi1|, max|psi2|, max|delta| and its 1-based index).

Two HIP models of this process are compared where their fields live (gb25_compare_field: one pass per field on the device,
nothing crosses PCIe); the record per field has the same keys and `ok` is the same norm test, from the sums the kernel returns.
Anything else (the CPU oracle, on_device=False) takes the numpy path.
"""
import math

import numpy as np


def norm_error(a, b):
    """(||a-b||_2, max(||a||_2, ||b||_2)): the two sides of Julia's isapprox for arrays."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a64 - b64).ravel())), float(max(np.linalg.norm(a64.ravel()),
                                                                   np.linalg.norm(b64.ravel())))


def approx_equal(a, b, rtol, atol):
    d, n = norm_error(a, b)
    if not np.isfinite(d):
        return False
    return bool(d <= max(atol, rtol * n))


def _compare(name, psi1, psi2, rtol, atol, out):
    """compare_parent / compare_interior (src/correctness.jl:4-26): psi1 may be smaller than psi2."""
    nx, ny, nz = psi1.shape
    psi2 = psi2[:nx, :ny, :nz]
    delta = np.abs(psi1.astype(np.float64) - psi2.astype(np.float64))
    idx = np.unravel_index(np.argmax(delta), delta.shape) if delta.size else (0, 0, 0)
    ok = approx_equal(psi1, psi2, rtol, atol)
    dn, nn = norm_error(psi1, psi2)
    rec = dict(name=name, ok=ok, rel=(dn / nn if nn > 0 else (0.0 if dn == 0 else float("inf"))), max1=float(np.max(np.abs(psi1))), max2=float(np.max(np.abs(psi2))),
               maxdelta=float(delta.max()) if delta.size else 0.0, index=tuple(int(i) + 1 for i in idx))
    out.append(rec)
    return ok


def _global_key(position, offset):
    """Memory order of the global array (i fastest): the sort key of a 1-based position placed by its global offset."""
    g = tuple(int(p) + int(o) for p, o in zip(position, offset))
    return (g[2], g[1], g[0]), g


def _best(records, value, position):
    """The largest value(record); ties: the smallest global linear offset.  Returns (value, global position)."""
    best = None
    for r in records:
        if not any(getattr(r, position)):     # (no such position: nothing finite on that rank)
            continue
        key, g = _global_key(getattr(r, position), r.global_offset)
        if best is None or value(r) > best[0] or (value(r) == best[0] and key < best[1]):
            best = (value(r), key, g)
    return (0.0, (0, 0, 0)) if best is None else (best[0], best[2])


def combine_stats(records):
    """The statistics of a global field from those of its ranks (binding.FieldStats of gb25_get_field_stats, interiors): min of
    mins, max of maxes, sums of sums and counts (in rank order), max|x| with the smallest GLOBAL linear offset on ties, the
    first non-finite value in global memory order.  Positions of the result are global (global_offset = 0)."""
    from .binding import FieldStats
    records = list(records)
    out = FieldStats()
    out.min, out.max = min(r.min for r in records), max(r.max for r in records)
    out.sum, out.sum_sq = math.fsum(r.sum for r in records), math.fsum(r.sum_sq for r in records)
    out.count, out.nonfinite = sum(r.count for r in records), sum(r.nonfinite for r in records)
    out.max_abs, at = _best(records, lambda r: r.max_abs, "at_max_abs")
    out.at_max_abs[:] = at
    bad = [_global_key(r.first_nonfinite, r.global_offset) for r in records if r.nonfinite]
    out.first_nonfinite[:] = min(bad)[1] if bad else (0, 0, 0)
    return out


def combine_diffs(records):
    """The same for binding.FieldDiff records of gb25_compare_field."""
    from .binding import FieldDiff
    records = list(records)
    out = FieldDiff()
    out.max_abs_a, out.max_abs_b = max(r.max_abs_a for r in records), max(r.max_abs_b for r in records)
    for k in ("sum_sq_a", "sum_sq_b", "sum_sq_delta"):
        setattr(out, k, math.fsum(getattr(r, k) for r in records))
    out.count, out.nonfinite = sum(r.count for r in records), sum(r.nonfinite for r in records)
    out.max_abs_delta, at = _best(records, lambda r: r.max_abs_delta, "at_max_abs_delta")
    out.at_max_abs_delta[:] = at
    return out


def diff_record(name, d, rtol, atol):
    """The report record of compare_states from a binding.FieldDiff: isapprox's norm test from the sums of squares."""
    dn, nn = math.sqrt(d.sum_sq_delta), max(math.sqrt(d.sum_sq_a), math.sqrt(d.sum_sq_b))
    finite = d.nonfinite == 0
    ok = bool(finite and dn <= max(atol, rtol * nn))
    rel = (dn / nn if nn > 0 else (0.0 if dn == 0 else float("inf"))) if finite else float("nan")
    return dict(name=name, ok=ok, rel=rel, max1=d.max_abs_a, max2=d.max_abs_b, maxdelta=d.max_abs_delta,
                index=tuple(int(i) for i in d.at_max_abs_delta))


def _device_pair(m1, m2):
    from .binding import HipBackend
    return isinstance(m1.backend, HipBackend) and isinstance(m2.backend, HipBackend)


def compare_states(m1, m2, *, rtol=None, atol=0.0, include_halos=False, throw_error=False, verbose=True, on_device=None):
    """compare_states(m1, m2; rtol=sqrt(eps(eltype(grid))), atol=0, include_halos, throw_error)
    -- src/correctness.jl:28-90.  Walks fields(model) = (u, v, w, eta, T, S), G^n and G^- of every name
    but w and eta, and the split-explicit filtered state (U, V, eta).  Returns (ok, report).
    on_device: None = on the device when both models are HIP models of this process (same or different float type), True =
    insist on it, False = download every field and compare with numpy."""
    if rtol is None:   # sqrt(eps(eltype(grid)))
        rtol = math.sqrt(np.finfo(getattr(m1.backend, "dtype", np.float32)).eps)
    if on_device is None:
        on_device = _device_pair(m1, m2)
    elif on_device and not _device_pair(m1, m2):
        raise TypeError("compare_states(on_device=True) needs two HIP models of this process")
    if on_device:
        # the fields stay where they are: `get` hands out the pair of Field objects, `compare` is one gb25_compare_field
        get = lambda f: f

        def compare(name, fa, fb, rtol, atol, out):
            d = fa._b.compare_field(fa.name, fb._b, include_halos, other_name=fb.name)
            out.append(diff_record(name, d, rtol, atol))
            return out[-1]["ok"]
    else:
        compare = _compare
        get = (lambda f: f.parent) if include_halos else (lambda f: f.interior)
    report, ok = [], True
    f1, f2 = m1.fields(), m2.fields()
    for name in f1:
        ok &= compare(name, get(f1[name]), get(f2[name]), rtol, atol, report)
        if name not in ("w", "eta"):
            ok &= compare(f"Gn.{name}", get(getattr(m1.timestepper.Gn, name)), get(getattr(m2.timestepper.Gn, name)),
                           rtol, atol, report)
            ok &= compare(f"Gm.{name}", get(getattr(m1.timestepper.Gm, name)), get(getattr(m2.timestepper.Gm, name)),
                           rtol, atol, report)
    for name in ("U", "V", "eta"):
        ok &= compare(f"filtered.{name}", get(getattr(m1.free_surface.filtered_state, name)),
                       get(getattr(m2.free_surface.filtered_state, name)), rtol, atol, report)
    # if m1.closure isa CATKEVerticalDiffusivity: the diffusivity fields (src/correctness.jl:60-67)
    if getattr(m1, "diffusivity_fields", None) is not None and getattr(m2, "diffusivity_fields", None) is not None:
        for name in ("kappa_u", "kappa_c", "kappa_e", "Le", "Jb"):
            ok &= compare(name, get(getattr(m1.diffusivity_fields, name)), get(getattr(m2.diffusivity_fields, name)),
                           rtol, atol, report)
    if verbose:
        for r in report:
            print("(%10s) psi1 ~ psi2: %-5s, max|psi1|, max|psi2|: %.9e, %.9e, max|d|: %.9e at %d %d %d"
                  % (r["name"], r["ok"], r["max1"], r["max2"], r["maxdelta"], *r["index"]))
    if not ok and throw_error:
        bad = [r["name"] for r in report if not r["ok"]]
        raise AssertionError(f"There is a discrepancy between the models: {bad} (rtol={rtol}, atol={atol})")
    return ok, report


def sync_states(m1, m2):
    """sync_states!(m1, m2): copy parent(field) of every field of m2 into m1 -- src/correctness.jl:92-103."""
    f1, f2 = m1.fields(), m2.fields()
    for name in f1:
        p2 = f2[name].parent
        nx, ny, nz = m1.backend.field_dims(f1[name].name, True)
        f1[name].set_parent(p2[:nx, :ny, :nz])
