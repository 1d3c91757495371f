"""A step is reproducible: identical models, built in one process from the same state and stepped by the same calls, hold the same
bits after every step -- every parent array of helpers.ALL_FIELDS (with CATKE: CATKE_FIELDS too), halos included, NaN equal to NaN.
Every bitwise tie of this suite (the routes, the tracer rows, the forms of the sub-cycle, "asking changes nothing") and every
"same bits" claim of a kernel change rests on this.  A result that depends on timing means two streams without an order, memory
read before it is written, or blocks of one launch that race; none of them shows in a norm-wise parity.

Matrix: Float32 and Float64; grids 0, 1, 3, 4 at helpers.size_of (48x24x6 is the smallest folded grid the sub-cycle accepts);
look-aheads none / sub-cycle alone / AB2 alone / both, without a closure, and CATKE on grids 0 and 4 with both.  Arrangements:

  interleaved    three models alive at once, stepping in turn (how the "asking changes nothing" tests run);
  in succession  build, step, download, close, then the next: the second model receives the first one's freed device memory, so a
                 kernel that reads what nothing wrote sees old field values, not fresh pages;
  single call    loop(m, 6) twice, and (w_on_the_fly = 0, where every route of a composite call promises the sweep's bits:
                 tests/test_gpu_step_routes.py) loop(m, 6) against six time_step calls;
  quiet pair     one model followed by synchronize() after every call, the other by nothing.

A download waits for the model, so a compare after every step could hide an ordering bug: the first two arrangements run twice,
comparing after every step and comparing only at the end.

Measured on an MI355X: the whole file (185 cases) takes 14 to 22 s.  What it found, and the counts of the cells that differed
before the fix, are in DESIGN.md, "Reproducibility of a step".
"""
import numpy as np
import pytest

import gb25_amd as gb
from helpers import ALL_FIELDS, CATKE_FIELDS, stepped_model

pytestmark = pytest.mark.gpu

STEPS = 6
LOOKAHEADS = {"none": dict(subcycle_lookahead=0, ab2_lookahead=0), "subcycle": dict(subcycle_lookahead=1, ab2_lookahead=0),
              "ab2": dict(subcycle_lookahead=0, ab2_lookahead=1), "both": dict(subcycle_lookahead=1, ab2_lookahead=1)}
CONFIGS = ([(ft, gt, la, False) for ft in ("Float32", "Float64") for gt in (0, 1, 3, 4) for la in LOOKAHEADS]
           + [(ft, gt, "both", True) for ft in ("Float32", "Float64") for gt in (0, 4)])
CONFIG_IDS = [f"{ft}-grid{gt}-{la}{'-catke' if catke else ''}" for ft, gt, la, catke in CONFIGS]
configs = pytest.mark.parametrize("float_type,grid_type,lookaheads,catke", CONFIGS, ids=CONFIG_IDS)
when = pytest.mark.parametrize("every_step", [True, False], ids=["each_step", "at_end"])


def names_of(catke):
    return ALL_FIELDS + (CATKE_FIELDS if catke else [])


def build(float_type, grid_type, lookaheads, catke, **more):
    closure = gb.CATKEVerticalDiffusivity() if catke else None
    return stepped_model(float_type, grid_type, steps=0, closure=closure, **dict(LOOKAHEADS[lookaheads], **more))


def download(model, names):
    return {n: model.backend.get_field(n, True) for n in names}


def difference(a, b, names):
    """None, or what the first field (in the order of `names`) that differs between the states a and b looks like."""
    for n in names:
        x, y = a[n], b[n]
        assert x.shape == y.shape and x.dtype == y.dtype, n
        bad = np.argwhere(~((x == y) | (np.isnan(x) & np.isnan(y))))
        if len(bad):
            with np.errstate(invalid="ignore"):
                delta = np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64)))
            others = [o for o in names[names.index(n) + 1:] if not np.array_equal(a[o], b[o], equal_nan=True)]
            return (f"{n}: {len(bad)} of {x.size} elements differ, first at {bad[0].tolist()}, last at {bad[-1].tolist()} "
                    f"(parent shape {list(x.shape)}), max |delta| {delta:.3g} of max |value| {np.nanmax(np.abs(y)):.3g}; "
                    f"later fields that differ: {', '.join(others) or 'none'}")
    return None


def assert_same(states, names, step, what):
    """states: one dict of downloaded fields per model; all must equal the first."""
    for q, s in enumerate(states[1:], 1):
        d = difference(states[0], s, names)
        assert d is None, f"{what}: after step {step} model {q} differs from model 0 in {d}"


@configs
@when
def test_interleaved(float_type, grid_type, lookaheads, catke, every_step):
    names = names_of(catke)
    models = [build(float_type, grid_type, lookaheads, catke) for _ in range(3)]
    try:
        if every_step:
            assert_same([download(m, names) for m in models], names, 0, "interleaved")
        for step in range(1, STEPS + 1):
            for m in models:
                gb.time_step(m)
            if every_step or step == STEPS:
                assert_same([download(m, names) for m in models], names, step, "interleaved")
    finally:
        for m in models:
            m.backend.close()


@configs
@when
def test_in_succession(float_type, grid_type, lookaheads, catke, every_step):
    names = names_of(catke)
    histories = []
    for _ in range(3):
        m = build(float_type, grid_type, lookaheads, catke)
        try:
            h = {0: download(m, names)} if every_step else {}
            for step in range(1, STEPS + 1):
                gb.time_step(m)
                if every_step or step == STEPS:
                    h[step] = download(m, names)
        finally:
            m.backend.close()
        histories.append(h)
    for step in sorted(histories[0]):
        assert_same([h[step] for h in histories], names, step, "in succession")


@configs
def test_single_call(float_type, grid_type, lookaheads, catke):
    names = names_of(catke)
    # the composite call as it is by default, twice
    a, b = (build(float_type, grid_type, lookaheads, catke) for _ in range(2))
    try:
        gb.loop(a, STEPS)
        gb.loop(b, STEPS)
        assert_same([download(a, names), download(b, names)], names, STEPS, "loop(6) twice")
    finally:
        a.backend.close()
        b.backend.close()
    # ... and against six calls, where the routes of a composite call promise the bits of the sweep
    a, b = (build(float_type, grid_type, lookaheads, catke, w_on_the_fly=0) for _ in range(2))
    try:
        gb.loop(a, STEPS)
        for _ in range(STEPS):
            gb.time_step(b)
        assert_same([download(b, names), download(a, names)], names, STEPS, "six time_step calls (model 0) against loop(6) (model 1)")
    finally:
        a.backend.close()
        b.backend.close()


@pytest.mark.parametrize("float_type,grid_type,catke", [("Float32", 0, False), ("Float32", 4, False), ("Float64", 4, False),
                                                         ("Float64", 3, False), ("Float32", 4, True)])
def test_a_synchronize_changes_no_bit(float_type, grid_type, catke):
    names = names_of(catke)
    quiet, loud = (build(float_type, grid_type, "both", catke) for _ in range(2))
    try:
        loud.backend.synchronize()
        for step in range(1, STEPS + 1):
            gb.time_step(quiet)
            gb.time_step(loud)
            loud.backend.synchronize()
        assert_same([download(quiet, names), download(loud, names)], names, STEPS, "quiet (model 0) against synchronised (model 1)")
    finally:
        quiet.backend.close()
        loud.backend.close()
