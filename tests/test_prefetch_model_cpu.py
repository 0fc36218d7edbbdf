"""The sequence atlas of tests/prefetch_model.py, checked on the host alone (no GPU): its data tell every two atmospheres apart
by a wide margin, it exercises every outcome and every route, and each of seven deliberately wrong models of the contract is
caught by a named step.  What the device does with the atlas is tests/test_prefetch_sequences.py."""
import functools

import numpy as np
import pytest

import numpy_oracle as npo
import prefetch_model as pm
import util
from coflux import interface_computations as ic
from coflux import synthetic as syn

FLUXES = ("sensible_heat", "latent_heat", "water_vapor", "x_momentum", "y_momentum")   # (the sixth interface field of the step is
# the interface temperature — the prescribed sea surface temperature here, whatever the atmosphere)
TILE = (20, 64, 32)     # the cells the margins are taken on: interior row, first interior column, columns
TH = 2                  # halo of a tile (≥ ring + 1)


@pytest.fixture(scope="module")
def cases():
    return [(name, mode, ops, pm.predict(mode, ops)) for name, mode, ops in pm.atlas()]


def _tile(a):
    """The tile of a parent-shaped array: one interior row and TILE[2] columns of the step shape, with a halo of TH."""
    j, i, n = TILE
    return a[pm.H + j - TH:pm.H + j + 1 + TH, pm.H + i - TH:pm.H + i + n + TH]


def _tile_map(name):
    w = pm.weights(name)
    shape = (pm.NY + 2 * pm.H, pm.NX + 2 * pm.H)
    fi = _tile(np.broadcast_to(w["fi"][None, :], shape) if w["separable"] else w["fi"])
    fj = _tile(np.broadcast_to(w["fj"][:, None], shape) if w["separable"] else w["fj"])
    return fi, fj, *(_tile(w[k]) if w.get(k) is not None else None for k in ("cos_rot", "sin_rot"))


@functools.lru_cache(maxsize=1)
def _band():
    """The source rows the tile reaches through any of the three maps (one band: the snapshots are generated once)."""
    fj = np.concatenate([_tile_map(name)[1].ravel() for name in pm.WEIGHTS])
    lo, hi, nsy = int(np.floor(fj.min())) - 1, int(np.ceil(fj.max())) + 2, pm.source_shape()[0]
    return (lo, hi) if lo >= 1 and hi <= nsy - 1 else (0, nsy)      # (a clamped row in reach: all rows)


def _tile_exchange(atmos):
    """The exchange fields of one Atmos on the tile, by the NumPy oracle from the source rows the tile reaches."""
    fi, fj, cs, sn = _tile_map(atmos.w)
    lo, hi = _band()
    a, b = pm.snapshot(atmos.src, *atmos.c1, lo, hi), pm.snapshot(atmos.src, *atmos.c2, lo, hi)
    src = {v: np.stack([a[v], b[v]]) for v in pm.VARIABLES}
    return npo.interpolate_atmosphere_state(src, fi, fj - lo, 0, 1, atmos.tf, cos_rot=cs, sin_rot=sn)


def _tile_fields(tuples, ocean):
    """Exchange fields and interface fluxes of every Atmos on the tile's ring window — the reference alone.  The solver runs
    once, on the tiles stacked into one tall surface (every tile brings its own halo rows: no cell sees another tile)."""
    at = [_tile_exchange(a) for a in tuples]
    tall = {k: np.concatenate([x[k] for x in at]) for k in EXCHANGE}
    oc = {k: np.concatenate([_tile(ocean[k])] * len(tuples)) for k in ("T", "S", "u", "v", "mask")}
    with np.errstate(all="ignore"):
        fl = npo.atmosphere_ocean_fluxes(ic.SimilarityTheoryFluxes(), oc, tall, hx=TH, hy=TH, ring=pm.RING,
                                         thermodynamics=ic.AtmosphereThermodynamicsParameters(), seawater=ic.SeawaterComposition(),
                                         ocean_properties=ic.OceanProperties())
    rows, win = 1 + 2 * TH, (slice(TH - pm.RING, TH + 1 + pm.RING), slice(TH - pm.RING, -(TH - pm.RING)))
    wet = (_tile(ocean["mask"])[win] != 0).ravel()
    assert wet.sum() > 40
    out = []
    for t, x in enumerate(at):
        f = {k: x[k][win].ravel() for k in EXCHANGE}
        for k in FLUXES:
            full = fl[k] if fl[k].shape == tall["T"].shape else np.pad(fl[k], TH - pm.RING)
            f["flux." + k] = full[t * rows:(t + 1) * rows][win].ravel()[wet]
        out.append(f)
    return out


EXCHANGE = ("u", "v", "T", "p", "q", "Qs", "Ql", "Mp")


def test_every_two_atmospheres_of_the_atlas_are_far_apart(cases):
    """§4 of the design: any two distinct Atmos tuples that any step of any case must see differ by ≥ 1e-3 in every exchange
    field and by ≥ 1e-6 in every interface flux, in the metric the device tests use (util.rel_err: the largest difference over
    the cells, relative to max(|reference|, field scale)).  Taken on 3 × 34 cells of the step shape with the NumPy oracle: the
    largest difference over a part of the cells bounds the one over all of them from below."""
    tuples = sorted({a for *_x, out in cases for o in out for a in o["sees"]}, key=repr)
    assert len(tuples) > 100
    ocean = syn.ocean_state(pm.NX, pm.NY, pm.H, pm.H)
    fields = _tile_fields(tuples, ocean)
    names = list(fields[0])
    worst = {}
    for k in names:
        X = np.stack([f[k] for f in fields])
        scale = util.ATMOS_SCALE[k] if k in util.ATMOS_SCALE and not k.startswith("flux.") else util.FIELD_SCALE[k[5:]]
        bound = 1e-6 if k.startswith("flux.") else 1e-3
        low = np.inf
        for i in range(len(tuples) - 1):
            d = np.max(np.abs(X[i + 1:] - X[i]) / np.maximum(np.abs(X[i]), scale), axis=1)
            j = int(np.argmin(d))
            if d[j] < low:
                low, worst[k] = float(d[j]), (tuples[i], tuples[i + 1 + j])
        assert low >= bound, (k, low, worst[k])


def test_the_atlas_reaches_every_outcome_every_route_and_every_mode_pair(cases):
    total = dict.fromkeys(pm.COUNTERS, 0)
    for _n, _m, _ops, out in cases:
        for k, v in out[-1]["counters"].items():
            total[k] += v
    for k in pm.ROUTES + pm.OUTCOMES + ("requests", "step_interpolations"):
        assert total[k] > 0, k
    assert any(o["refused"] for *_x, out in cases for o in out)
    # all nine (mode at the request, mode when it leaves or is consumed) pairs, in named cases
    pairs = set()
    for name, mode, ops, _out in cases:
        if name.startswith("walk"):
            continue
        at_request = None
        for op in ops:
            if isinstance(op, pm.SetMode):
                mode = op.mode
            elif isinstance(op, pm.Request):
                at_request = mode
            elif isinstance(op, pm.Step) and at_request is not None:
                pairs.add((at_request, mode))
    assert pairs == {(a, b) for a in range(3) for b in range(3)}
    # every case that voids a request goes on to step into the voided set
    for name, mode, ops, out in cases:
        voided_sets, m = set(), pm.Model(mode)
        for op in ops:
            before = dict(m.pending)
            m.apply(op)
            if isinstance(op, pm.Commit):
                voided_sets |= {s for s in before if s not in m.pending}
            elif isinstance(op, pm.Step):
                voided_sets.discard(op.set)
            elif isinstance(op, pm.TimeSteps):
                voided_sets -= {"A", "B"}
        assert name.startswith("walk") or not voided_sets, (name, voided_sets)


def test_the_walks_are_legal_long_and_reproducible():
    assert len(pm.WALK_SEEDS) == 24
    for seed in pm.WALK_SEEDS:
        mode, ops = pm.walk(seed)
        assert mode == seed % 3 and len(ops) == pm.WALK_LENGTH and (mode, ops) == pm.walk(seed)
        assert any(isinstance(op, pm.SetMode) for op in ops) or seed not in (0, 1, 2)
        pm.predict(mode, ops)      # raises on an illegal operation or a broken invariant
    assert sum(pm.walk(s)[0] == 0 for s in pm.WALK_SEEDS) == 8
    with pytest.raises(pm.ContractViolation):     # the host writes a set a request is pending for
        pm.predict(0, [pm.R("A", pm.K0), pm.Write("A", "W", "lat", *pm.K1)])


CAUGHT_BY = {
    "ignore_commits": ("commit_voids_aux", "commit_voids_deferred", "commit_voids_on_main", "continuing_split_recommit_8_1_12",
                       "ice_tail_commit_voids_deferred", "ice_tail_commit_voids_tail"),
    "ignore_fraction": ("time_mismatch", "continuing_split_clock_change_8_1_12", "continuing_split_clock_and_mode_change_0to1_8_1_12",
                        "continuing_split_clock_and_mode_change_0to2_8_1_12", "request_into_current_set", "ice_tail_time_mismatch"),
    "ignore_source": ("source_mismatch", "continuing_split_source_change_8_1_12"),
    "ignore_weights": ("weights_mismatch", "continuing_split_weights_change_8_1_12"),
    "discard_forgets_deferred_only": ("discard_aux", "discard_on_main", "continuing_stop_discard"),
    "supersede_keeps_old": ("supersede_then_old_clock",),
    "continuing_trusts_pending": ("continuing_split_clock_change_8_1_12", "continuing_split_source_change_8_1_12",
                                  "continuing_split_weights_change_8_1_12", "continuing_split_clock_and_mode_change_0to1_8_1_12",
                                  "continuing_split_clock_and_mode_change_0to2_8_1_12"),
}


def observed(out):
    """What the device test compares: of every operation the step whose outputs are still there afterwards — its last."""
    return [o["sees"][-1:] for o in out]


@pytest.mark.parametrize("defect", pm.DEFECTS)
def test_each_wrong_model_predicts_another_atmosphere_for_a_named_step(cases, defect):
    """Seeded defects, as in test_regime_atlas.py: a model that ignores commits / the fraction / the source / the weights in its
    key, whose discard forgets only the request that has not left, whose supersede keeps the old record, or whose continuing
    call trusts whatever is pending, must disagree with the contract's model on the atmosphere of a step the device test
    compares — the LAST step of an operation: what an inner step of a cf_time_steps call computed is overwritten before the call
    returns — else no device test could tell a library with that defect from a sound one by its numbers.  Caught by (each in
    every mode it runs in):
      ignore_commits                 commit_voids_aux / _deferred / _on_main, continuing_split_recommit_8_1_12, ice_tail_commit_voids_*
      ignore_fraction                time_mismatch, continuing_split_clock_change_8_1_12, _clock_and_mode_change_0to1/2_8_1_12,
                                     request_into_current_set, ice_tail_time_mismatch
      ignore_source                  source_mismatch, continuing_split_source_change_8_1_12
      ignore_weights                 weights_mismatch, continuing_split_weights_change_8_1_12
      discard_forgets_deferred_only  discard_aux, discard_on_main, continuing_stop_discard (not discard_deferred: nothing has left)
      supersede_keeps_old            supersede_then_old_clock
      continuing_trusts_pending      continuing_split_clock_change / _source_change / _weights_change / _clock_and_mode_change, all _8_1_12
    and by several walks each.  The 8 + 13 forms of the continuing cases differ at an inner step only (asserted below): on the
    device they are held by the counters and by the call's last step, their 8 + 1 + 12 twins by the numbers of step 8."""
    caught = set()
    for name, mode, ops, out in cases:
        wrong = pm.predict(mode, ops, defects=(defect,))
        if observed(out) != observed(wrong):
            caught.add(name.split("/")[0])
    named = {c for c in caught if not c.startswith("walk")}
    assert named, defect
    assert set(CAUGHT_BY[defect]) <= named, (defect, sorted(set(CAUGHT_BY[defect]) - named))
    assert not any(c.startswith("continuing_split") and not c.endswith("_8_1_12") for c in named), sorted(named)
