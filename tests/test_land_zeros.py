"""CF_OPT_LAND_ZEROS (include/coflux.h): inside cf_time_steps only the call's first step writes zero_interface_state into the
land cells; later steps leave them alone (csrc/coflux_lean_kernel.hpp and csrc/coflux_solver.hip: `keep_land` in the start
phase; csrc/coflux_net.hip: net_stress_kernel; csrc/coflux_abi.cpp: update_state_impl decides, csrc/coflux_ctx.hpp:
LandZeroScope bounds the decision to one call).

Shape `base` of tests/mask_atlas.py (131 × 37, halo 3, ring 1, about 21 chunks), the masks blob, checkerboard, ring_only,
interior_only, single_last and the two with a land run of 3000 cells (longer than the 8 × 256 strips a workgroup requests up
front: the loop behind them), both mask kinds, the presets :default and :corrected (the lean body) and :ncar (the fast body),
each with the net fluxes fused into the solver launch and not.

Every comparison is of BITS, on the whole array (halos included), so there is no tolerance to state.  Outputs start as
7.0e77 (`iterations` as util.SENTINEL32); the documented footprint is the ring-inclusive window for the flux fields and the
interior for the net fields.

One thing the skipping branch cannot leave as it is, by construction, and test 1 states it instead of hiding it: a wet
interior cell's face stress averages ρτ with its west / south neighbour's.  Under the experiment value 2 a land neighbour's ρτ
is not written, so the wet cell's τ is the average with whatever the land cell held — here the sentinel.  (In the automatic
mode the land cell holds the first step's zero, which is why tests 2-4 can ask for whole-array equality.)  Test 1 therefore
holds τx, τy of wet cells to the kernel's own arithmetic, restated in NumPy and first shown to reproduce the every-launch run
bit for bit: equal to the every-launch run wherever the face neighbour is wet, the stated average elsewhere.  Every other
field of every wet cell must be the every-launch run's bits."""
import os
import re

import numpy as np
import pytest

import mask_atlas as ma
import util
from coflux import abi
from coflux import interface_computations as ic
from coflux.runtime import EXCHANGE_NAMES, FLUX_NAMES, FLUX_OPTIONAL, NET_NAMES

gpu = pytest.mark.gpu

H, RING = ma.HALO, ma.RING
SHAPE = "base"
NX, NY = ma.SHAPES[SHAPE]
MASKS = ("blob", "checkerboard", "ring_only", "interior_only", "single_last", "land_run_then_wet", "wet_then_land_run")
KINDS = ("u8", "bottom_height")
PRESETS = ("default", "corrected", "ncar")
CELL_FIELDS = FLUX_NAMES + FLUX_OPTIONAL
SENTINEL = 7.0e77
N_LEVELS, INC = 4, 1.0 / 9.0


def test_the_option_and_the_hook_are_mirrored():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "coflux.h")).read()
    assert re.search(r"^#define CF_OPT_LAND_ZEROS %d\b" % abi.OPT_LAND_ZEROS, header, flags=re.M)
    assert (abi.LAND_ZEROS_EVERY_LAUNCH, abi.LAND_ZEROS_AUTO, abi.LAND_ZEROS_NEVER) == (0, 1, 2)
    assert "cf_debug_land_zero_launches" in abi.EXPORTED_SYMBOLS and hasattr(abi.load_library(), "cf_debug_land_zero_launches")


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def _params(preset, kind):
    fluxes, vd = util.CONFIGS[preset]()
    return ic.flux_params(fluxes, velocity_difference=vd, mask_kind=abi.MASK_BOTTOM_HEIGHT if kind == "bottom_height" else abi.MASK_U8)


def _wet(name):
    wx, wy = ma.window_shape(NX, NY, RING)
    return dict(ma.atlas(wx, wy, only=(name,)))[name]


def _sentinel_outputs(ctx):
    import torch
    fl = {k: torch.full(ctx.shape, SENTINEL, dtype=torch.float64, device=ctx.device) for k in CELL_FIELDS}
    fl["iterations"] = util._fill(torch.empty(ctx.shape, dtype=torch.int32, device=ctx.device), util.SENTINEL32)
    net = {k: torch.full(ctx.shape, SENTINEL, dtype=torch.float64, device=ctx.device) for k in NET_NAMES}
    return fl, net


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def _is_sentinel(a):
    return a == np.int32(util.SENTINEL32) if a.dtype == np.int32 else _bits(a) == _bits(np.array([SENTINEL]))[0]


def _same(label, got, ref):
    for k in ref:
        diff = _bits(got[k]) != _bits(ref[k])
        assert not diff.any(), (label, k, "cells differ", int(diff.sum()), np.argwhere(diff)[:4].tolist())


def _no_sentinel_in_footprint(label, fl, net):
    for k, a in fl.items():
        left = int(_is_sentinel(util.window(a, H, H, NX, NY, RING)).sum())
        assert left == 0, (label, k, "window cells left unwritten", left)
    for k, a in net.items():
        left = int(_is_sentinel(util.window(a, H, H, NX, NY, 0)).sum())
        assert left == 0, (label, "net." + k, "interior cells left unwritten", left)


class _Rig:
    """One context with the ocean states, the snapshots and the weights of shape `base` on the device."""

    def __init__(self, preset, kind, fused=True):
        from coflux import synthetic as syn
        from coflux.runtime import FluxContext
        self.kind = kind
        self.params = _params(preset, kind)
        self.ctx = ctx = FluxContext(NX, NY, H, H, self.params, ring=RING)
        if not fused:
            ctx.set_option(abi.OPT_FUSED_NET, 0)
        assert ctx.solver_path() == (preset != "ncar", 1 if fused else 0)   # lean / fast body, fused or not: what the case is for
        o0 = util.build_case(NX, NY, H, H, land=False)["ocean"]
        o1 = syn.evolved_ocean_state(o0, NX, NY, H, H, 1)
        self.oceans = [{k: ctx.to_device(o[k]) for k in ("T", "S", "u", "v")} for o in (o0, o1)]
        self.src = {k: ctx.to_device(v) for k, v in syn.jra55_snapshots(N_LEVELS).items()}
        fi, fj, phi = syn.latlon_fractional_indices(NX, NY, H, H)
        self.w = dict(separable=True, fi=ctx.to_device(fi), fj=ctx.to_device(fj), latitude=ctx.to_device(phi))
        self.keep = []

    def mask(self, wet):
        self.keep.append(self.ctx.to_device(ma.embed(wet, NX, NY, kind=self.kind)))   # a fresh pointer: the table is rebuilt
        return self.keep[-1]

    def states(self, mask):
        return [dict(o, mask=mask) for o in self.oceans]

    def host_step(self, s, states, atmos, fl, net):
        tot = s * INC
        l1 = int(tot) % N_LEVELS
        self.ctx.update_state(self.src, self.w, states[s % 2], atmos, fl, net, level1=l1, level2=(l1 + 1) % N_LEVELS,
                              time_fraction=tot - int(tot))

    def loop(self, first, n, states, sets, fl, net, pipeline):
        sched = self.ctx.make_schedule(states, sets, first_level=0, time_fraction=0.0, time_fraction_increment=INC, pipeline=pipeline)
        self.ctx.time_steps(first, n, sched, self.src, self.w, fl, net)

    def sets(self, pipeline):
        return [self.ctx.field_set(EXCHANGE_NAMES) for _ in range(2 if pipeline else 1)]

    def done(self):
        import torch
        self.ctx.sync()
        torch.cuda.synchronize()


def _face_stress(rho_tau, shift_axis, rho_o_inv):
    """net_face_stress without sea ice, contraction off: ((1 − 0)·(½(ρτ_a + ρτ_b)·ρₒ⁻¹)) + 0·0, a = the west / south neighbour."""
    a = np.roll(rho_tau, 1, axis=shift_axis)
    with np.errstate(over="ignore"):
        tao = 0.5 * (a + rho_tau) * rho_o_inv
        return (1.0 - 0.0) * tao + 0.0 * 0.0


# ---------------------------------------------------------------------------------------------
# 1. the skipping branch itself: one launch under the experiment value
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("preset", PRESETS)
def test_one_launch_that_never_writes_land_leaves_it_and_nothing_else(preset, kind, fused):
    """cf_update_state once under CF_OPT_LAND_ZEROS = 2 into sentinel-filled outputs, against the same under 0.  Land of the
    window (flux fields, `iterations`) and, fused, of the interior (every net field, τx and τy included) still holds the sentinel;
    un-fused the stand-alone net-flux kernel does not know the option and writes its land; every other cell of every array is
    the every-launch run's, bit for bit — wet cells, and whatever lies outside the footprint — with τx, τy of wet cells as the
    module docstring says."""
    rig = _Rig(preset, kind, fused)
    ctx = rig.ctx
    rinv = 1.0 / rig.params.ocean_reference_density
    for name in MASKS:
        wet, label = _wet(name), (preset, kind, fused, name)
        mask = rig.mask(wet)
        oc = rig.states(mask)[0]
        runs = {}
        for value in (abi.LAND_ZEROS_EVERY_LAUNCH, abi.LAND_ZEROS_NEVER):
            ctx.set_option(abi.OPT_LAND_ZEROS, value)
            fl, net = _sentinel_outputs(ctx)
            atmos = ctx.field_set(EXCHANGE_NAMES)
            ctx.update_state(rig.src, rig.w, oc, atmos, fl, net, level1=0, level2=1, time_fraction=0.37)
            rig.done()
            runs[value] = (_host(fl), _host(net))
        (fl0, net0), (fl2, net2) = runs[abi.LAND_ZEROS_EVERY_LAUNCH], runs[abi.LAND_ZEROS_NEVER]
        _no_sentinel_in_footprint(label + ("every launch",), fl0, net0)
        land_w = np.zeros(ctx.shape, bool)
        util.window(land_w, H, H, NX, NY, RING)[...] = ~wet
        land_i = np.zeros(ctx.shape, bool)
        util.window(land_i, H, H, NX, NY, 0)[...] = ~util.window(wet, RING, RING, NX, NY, 0)
        wet_i = np.zeros(ctx.shape, bool)
        util.window(wet_i, H, H, NX, NY, 0)[...] = util.window(wet, RING, RING, NX, NY, 0)
        # the flux fields: land of the window untouched, everything else the every-launch run
        expect = {k: np.where(land_w, np.array(SENTINEL if a.dtype == np.float64 else util.SENTINEL32, dtype=a.dtype), a) for k, a in fl0.items()}
        _same(label + ("fluxes",), fl2, expect)
        # the restated face stress reproduces the every-launch run on wet cells, bit for bit …
        for k, rt, axis in (("u", "x_momentum", 1), ("v", "y_momentum", 0)):
            model0 = _face_stress(fl0[rt], axis, rinv)
            assert np.array_equal(_bits(model0[wet_i]), _bits(net0[k][wet_i])), (label, "net." + k, "the restated face stress is not the kernel's")
        # … so it says what a wet cell beside untouched land must hold
        expect = {}
        for k, a in net0.items():
            e = np.where(land_i, SENTINEL, a) if fused else a.copy()
            if k in ("u", "v"):
                rt, axis = ("x_momentum", 1) if k == "u" else ("y_momentum", 0)
                e[wet_i] = _face_stress(fl2[rt], axis, rinv)[wet_i]
                neighbour_wet = wet_i & np.roll(~land_w, 1, axis=axis)
                assert np.array_equal(_bits(e[neighbour_wet]), _bits(a[neighbour_wet])), (label, k)   # the every-launch bits wherever no land is read
            expect[k] = e
        _same(label + ("net",), net2, expect)
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 2. the loop
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("pipeline", [True, False], ids=["tail", "unpipelined"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("preset", PRESETS)
def test_four_steps_are_the_every_launch_loop_and_the_host_loop_bitwise(preset, kind, pipeline, fused):
    """cf_time_steps, 4 steps into sentinel-filled outputs, automatic mode == the same call under CF_OPT_LAND_ZEROS = 0 == a host
    loop of cf_update_state: the six flux fields, the similarity scales, `iterations` and all eight net fields on the whole array,
    no sentinel left inside the footprint; one solver launch of the automatic call carried the zeros, four of the other.
    `tail`: CF_OPT_MERGED_PREFETCH = 2 with two exchange sets — fused, steps 0-2 carry the next step's interpolation in tail
    workgroups and step 3 does not; un-fused, the interpolation goes out as a launch of its own."""
    n = 4
    rig = _Rig(preset, kind, fused)
    ctx = rig.ctx
    for name in MASKS:
        label = (preset, kind, pipeline, fused, name)
        states = rig.states(rig.mask(_wet(name)))
        ctx.set_option(abi.OPT_MERGED_PREFETCH, 0)
        ctx.set_option(abi.OPT_LAND_ZEROS, abi.LAND_ZEROS_AUTO)
        ref_fl, ref_net = _sentinel_outputs(ctx)
        ref_atmos = ctx.field_set(EXCHANGE_NAMES)
        for s in range(n):
            rig.host_step(s, states, ref_atmos, ref_fl, ref_net)
        rig.done()
        if pipeline:
            ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
        got = {}
        for value in (abi.LAND_ZEROS_AUTO, abi.LAND_ZEROS_EVERY_LAUNCH):
            ctx.set_option(abi.OPT_LAND_ZEROS, value)
            fl, net = _sentinel_outputs(ctx)
            rig.loop(0, n, states, rig.sets(pipeline), fl, net, pipeline)
            rig.done()
            got[value] = (_host(fl), _host(net))
            assert ctx.debug_land_zero_launches() == (1 if value == abi.LAND_ZEROS_AUTO else n), (label, value)
        (fl1, net1), (fl0, net0) = got[abi.LAND_ZEROS_AUTO], got[abi.LAND_ZEROS_EVERY_LAUNCH]
        _no_sentinel_in_footprint(label, fl1, net1)
        _same(label + ("fluxes vs every launch",), fl1, fl0)
        _same(label + ("net vs every launch",), net1, net0)
        _same(label + ("fluxes vs host loop",), fl1, _host(ref_fl))
        _same(label + ("net vs host loop",), net1, _host(ref_net))
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 3. a stale list
# ---------------------------------------------------------------------------------------------
STALE = {"blob_shifted": ("blob", None), "land_run_swapped": ("land_run_then_wet", "wet_then_land_run"),
         "checkerboard_inverted": ("checkerboard", None)}


@gpu
@pytest.mark.parametrize("case", list(STALE))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("preset", PRESETS)
def test_a_mask_rewritten_in_place_costs_time_never_land_zeros(preset, kind, case):
    """The chunk table and its lists are built for one mask and an earlier call leaves that mask's fluxes in the outputs; then the
    mask is rewritten behind the same pointer — wet cells become land, land cells wet (the blob moved by five columns, the
    checkerboard inverted, the 3000-cell land run moved from the head of the window to its tail: the loop behind the strips
    skips its zeros and the fingerprint then fails).  Three steps of cf_time_steps, automatic == CF_OPT_LAND_ZEROS = 0 on the whole
    array, and the new land holds zero_interface_state, not the earlier call's fluxes."""
    import torch
    old_name, new_name = STALE[case]
    old = _wet(old_name)
    new = _wet(new_name) if new_name else (np.roll(old, 5, axis=1) if case == "blob_shifted" else ~old)
    assert (old & ~new).any() and (~old & new).any()
    rig = _Rig(preset, kind)
    ctx = rig.ctx
    got = {}
    for value in (abi.LAND_ZEROS_AUTO, abi.LAND_ZEROS_EVERY_LAUNCH):
        ctx.set_option(abi.OPT_LAND_ZEROS, value)
        mask = rig.mask(old)
        states = rig.states(mask)
        ctx.ensure_chunk_table(mask)
        fl, net = _sentinel_outputs(ctx)
        sets = rig.sets(False)
        rig.loop(0, 2, states, sets, fl, net, False)          # the earlier call: the old mask's fluxes
        rig.done()
        assert np.count_nonzero(util.window(fl["latent_heat"].cpu().numpy(), H, H, NX, NY, RING)[old & ~new]) > 0
        mask.copy_(torch.as_tensor(ma.embed(new, NX, NY, kind=kind)).to(mask.device))   # same pointer, the table is not rebuilt
        rig.loop(2, 3, states, sets, fl, net, False)
        rig.done()
        got[value] = (_host(fl), _host(net))
        assert ctx.debug_land_zero_launches() == (1 if value == abi.LAND_ZEROS_AUTO else 3)
    (fl1, net1), (fl0, net0) = got[abi.LAND_ZEROS_AUTO], got[abi.LAND_ZEROS_EVERY_LAUNCH]
    label = (preset, kind, case)
    _same(label + ("fluxes",), fl1, fl0)
    _same(label + ("net",), net1, net0)
    _no_sentinel_in_footprint(label, fl1, net1)
    new_land = old & ~new
    for k in CELL_FIELDS:
        cells = util.window(fl1[k], H, H, NX, NY, RING)[new_land]
        assert np.all(cells == (-273.15 if k == "temperature" else 0.0)), (label, k, "new land holds an earlier call's values")
    new_land_i = util.window(new_land, RING, RING, NX, NY, 0)
    for k in NET_NAMES:
        assert not np.any(util.window(net1[k], H, H, NX, NY, 0)[new_land_i]), (label, "net." + k)
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 4. scope: what a cf_time_steps call decides ends with the call
# ---------------------------------------------------------------------------------------------
def _host_update_writes_every_land_zero(rig, states, label):
    """A host cf_update_state into fresh sentinel-filled outputs == the same under CF_OPT_LAND_ZEROS = 0, nothing left unwritten."""
    ctx = rig.ctx
    got = {}
    for value in (abi.LAND_ZEROS_AUTO, abi.LAND_ZEROS_EVERY_LAUNCH):   # (automatic first: the state under test is the one the loop left)
        ctx.set_option(abi.OPT_LAND_ZEROS, value)
        fl, net = _sentinel_outputs(ctx)
        rig.host_step(5, states, ctx.field_set(EXCHANGE_NAMES), fl, net)
        rig.done()
        got[value] = (_host(fl), _host(net))
    ctx.set_option(abi.OPT_LAND_ZEROS, abi.LAND_ZEROS_AUTO)
    _no_sentinel_in_footprint(label, *got[abi.LAND_ZEROS_AUTO])
    _same(label + ("fluxes",), got[abi.LAND_ZEROS_AUTO][0], got[abi.LAND_ZEROS_EVERY_LAUNCH][0])
    _same(label + ("net",), got[abi.LAND_ZEROS_AUTO][1], got[abi.LAND_ZEROS_EVERY_LAUNCH][1])


@gpu
@pytest.mark.parametrize("preset", ["default", "ncar"])
def test_the_mark_does_not_outlive_a_call(preset):
    """After a cf_time_steps call a host cf_update_state writes every land zero; so it does after a call that is refused for what
    its second step would read (ocean state 1 without a temperature field: the whole call is refused before its first launch,
    and the step loop is never opened)."""
    from coflux.runtime import CofluxError
    rig = _Rig(preset, "u8")
    ctx = rig.ctx
    states = rig.states(rig.mask(_wet("blob")))
    fl, net = _sentinel_outputs(ctx)
    rig.loop(0, 4, states, rig.sets(False), fl, net, False)
    rig.done()
    _host_update_writes_every_land_zero(rig, states, (preset, "after a call"))
    broken = [states[0], dict(states[1], T=None)]
    with pytest.raises(CofluxError, match="ocean surface fields are NULL"):
        rig.loop(0, 4, broken, rig.sets(False), fl, net, False)
    rig.done()
    assert ctx.debug_land_zero_launches() == 1          # (the count of the call before: the refused one opened no loop)
    _host_update_writes_every_land_zero(rig, states, (preset, "after a failed call"))
    ctx.close()


@gpu
@pytest.mark.parametrize("pipeline", [True, False], ids=["tail", "unpipelined"])
@pytest.mark.parametrize("preset", ["default", "ncar"])
def test_every_call_starts_over(preset, pipeline):
    """Two consecutive cf_time_steps calls, the outputs sentinel-filled in between: the second call's first step writes the land
    again — each call's result is the every-launch loop's, whole array."""
    rig = _Rig(preset, "bottom_height")
    ctx = rig.ctx
    if pipeline:
        ctx.set_option(abi.OPT_MERGED_PREFETCH, 2)
    states = rig.states(rig.mask(_wet("land_run_then_wet")))
    got = {}
    for value in (abi.LAND_ZEROS_AUTO, abi.LAND_ZEROS_EVERY_LAUNCH):
        ctx.set_option(abi.OPT_LAND_ZEROS, value)
        sets, calls = rig.sets(pipeline), []
        for first, n in ((0, 3), (3, 2)):
            fl, net = _sentinel_outputs(ctx)
            rig.loop(first, n, states, sets, fl, net, pipeline)
            rig.done()
            calls.append((_host(fl), _host(net)))
            assert ctx.debug_land_zero_launches() == (1 if value == abi.LAND_ZEROS_AUTO else n)
        got[value] = calls
    for c in range(2):
        label = (preset, pipeline, "call", c)
        _no_sentinel_in_footprint(label, *got[abi.LAND_ZEROS_AUTO][c])
        _same(label + ("fluxes",), got[abi.LAND_ZEROS_AUTO][c][0], got[abi.LAND_ZEROS_EVERY_LAUNCH][c][0])
        _same(label + ("net",), got[abi.LAND_ZEROS_AUTO][c][1], got[abi.LAND_ZEROS_EVERY_LAUNCH][c][1])
    ctx.close()


# ---------------------------------------------------------------------------------------------
# 5. host bookkeeping
# ---------------------------------------------------------------------------------------------
@gpu
def test_how_many_launches_carried_the_zeros():
    """cf_debug_land_zero_launches: 0 before any call, 1 of n ≥ 1 steps under the automatic mode, n under CF_OPT_LAND_ZEROS = 0,
    pipelined or not; the experiment value 2 is refused outside an experiment process and counts 0 inside one; 3 is no value."""
    from coflux.runtime import CofluxError
    rig = _Rig("default", "u8")
    ctx = rig.ctx
    assert ctx.debug_land_zero_launches() == 0
    states = rig.states(rig.mask(_wet("blob")))
    fl, net = _sentinel_outputs(ctx)
    for pipeline in (False, True):
        ctx.set_option(abi.OPT_MERGED_PREFETCH, 2 if pipeline else 0)
        sets = rig.sets(pipeline)
        for n in (1, 2, 5):
            for value, want in ((abi.LAND_ZEROS_AUTO, 1), (abi.LAND_ZEROS_EVERY_LAUNCH, n)):
                ctx.set_option(abi.OPT_LAND_ZEROS, value)
                rig.loop(0, n, states, sets, fl, net, pipeline)
                assert ctx.debug_land_zero_launches() == want, (pipeline, n, value)
    with pytest.raises(CofluxError, match="land zeros 3"):
        ctx.set_option(abi.OPT_LAND_ZEROS, 3)
    if os.environ.get("COFLUX_EXPERIMENTS") == "1":
        ctx.set_option(abi.OPT_LAND_ZEROS, abi.LAND_ZEROS_NEVER)
        rig.loop(0, 2, states, rig.sets(False), fl, net, False)
        assert ctx.debug_land_zero_launches() == 0
    else:
        with pytest.raises(CofluxError, match="experiment value"):
            ctx.set_option(abi.OPT_LAND_ZEROS, abi.LAND_ZEROS_NEVER)
    rig.done()
    ctx.close()
