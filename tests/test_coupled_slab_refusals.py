"""cf_time_steps_coupled under CF_HALO_PEER in one process (include/coflux.h): what it refuses, by name and with the outputs and
the exchange count untouched, and that the accepted call computes what CF_HALO_NONE computes.  The context is connected as rank
0 of 1 in both worlds — the halo mailboxes and the reduction world of the exact sums — so that nothing can wait: the device of
tests/test_refused_step_calls.py.  The slabs themselves are tests/test_coupled_slabs.py's."""
import pytest
import torch

import test_coupled_steps as tcs
from coflux import abi
from coflux.runtime import CofluxError

pytestmark = pytest.mark.gpu

ROWS, STEPS = 2, 7          # halo_rows = ring + 1
SHAPE = (131, 37, 4, 3)


def rig_with(halo=None, reduce=False):
    """a context on the designed case; `halo`: max_fields of a halo mailbox connected as rank 0 of 1; `reduce`: a world of one"""
    rig = tcs.Rig(tcs.host_case(*SHAPE), merged=2)
    if halo is not None:
        rig.ctx.peer_halo_export(halo, ROWS)
        rig.ctx.peer_halo_connect(None, None, 0, 1)
    if reduce:
        rig.ctx.peer_reduce_export()
        rig.ctx.peer_reduce_connect(None, 0, 1)
    return rig


def arguments(rig, out, *, backend=abi.HALO_PEER, normalize="exact", pipeline=abi.PIPELINE_WITHIN_CALL):
    sch, block = tcs.coupled_arguments(rig, out, pipeline=pipeline, normalize=normalize)
    sch.halo_backend, sch.halo_rows = backend, ROWS if backend != abi.HALO_NONE else 0
    return sch, block


def test_every_refusal_names_its_field_and_the_accepted_call_is_the_single_domain():
    full, bare, small, no_world = rig_with(8, True), rig_with(), rig_with(4, True), rig_with(8, False)
    rigs = (full, bare, small, no_world)
    try:
        out = tcs.Outputs(full)
        untouched = out.bits()

        def refused(rig, *names, starts=None, mutate=None, **kw):
            sch, block = arguments(rig, out, **kw)
            if mutate is not None:
                mutate(sch, block)
            before = rig.ctx.peer_halo_stats()
            with pytest.raises(CofluxError) as err:
                rig.ctx.time_steps_coupled(0, STEPS, sch, rig.src, rig.w, out.fl, out.net, rig.stresses, block)
            text = str(err.value)
            assert "(-1)" in text and all(n in text for n in names), (names, text)
            if starts:
                assert text.split("): ", 1)[1].startswith(starts), text
            rig.ctx.sync()
            tcs.assert_same_bits(out.bits(), untouched, f"refused for {names}")
            assert rig.ctx.peer_halo_stats() == before == (0, 0), names

        refused(full, "halo_backend", "exercised", backend=abi.HALO_RCCL)
        refused(bare, "halo_backend", "cf_peer_halo_connect", starts="cf_time_steps_coupled: halo_backend = ")
        # nine fields per step (four ocean, five of the ice state) are exchanges of eight and one: a mailbox of four is too small
        refused(small, "halo_backend", "8 fields", starts="cf_time_steps_coupled: halo_backend = ")
        refused(full, "normalize_salinity", "slab", normalize=True)
        refused(no_world, "cf_peer_reduce_connect")
        for value in (-1, 3):
            refused(full, "normalize_salinity", mutate=lambda sch, block, v=value: setattr(block, "normalize_salinity", v))
            refused(full, "normalize_salinity", backend=abi.HALO_NONE, mutate=lambda sch, block, v=value: setattr(block, "normalize_salinity", v))
        refused(full, "fold_north", mutate=lambda sch, block: setattr(sch, "fold_north", 1))

        # … and the same call is accepted: seven steps under CF_HALO_PEER leave the bits of the CF_HALO_NONE run, whole buffers
        want = tcs.Outputs(full)
        sch, block = arguments(full, want, backend=abi.HALO_NONE)
        full.ctx.time_steps_coupled(0, STEPS, sch, full.src, full.w, want.fl, want.net, full.stresses, block)
        full.ctx.sync()
        assert full.ctx.peer_halo_stats() == (0, 0)
        sch, block = arguments(full, out)
        full.ctx.time_steps_coupled(0, STEPS, sch, full.src, full.w, out.fl, out.net, full.stresses, block)
        full.ctx.sync()
        tcs.assert_same_bits(out.bits(), want.bits(), "CF_HALO_PEER on a world of one")
        assert not torch.equal(out.bits()["net.S"], untouched["net.S"])
        # the stresses and the skin temperature once, then per step nine fields as two exchanges; none rode in a solver launch
        assert full.ctx.peer_halo_stats() == (1 + 2 * STEPS, 0)
        # CF_OPT_HALO_IN_SOLVER_LAUNCH arms no request in the coupled form: same bits, same count, and a plain step afterwards
        # finds nothing armed
        full.ctx.set_option(abi.OPT_HALO_IN_SOLVER_LAUNCH, 1)
        again = tcs.Outputs(full)
        sch, block = arguments(full, again)
        full.ctx.time_steps_coupled(0, STEPS, sch, full.src, full.w, again.fl, again.net, full.stresses, block)
        full.ctx.sync()
        tcs.assert_same_bits(again.bits(), want.bits(), "with CF_OPT_HALO_IN_SOLVER_LAUNCH")
        assert full.ctx.peer_halo_stats() == (2 * (1 + 2 * STEPS), 0)
    finally:
        for rig in rigs:
            rig.close()


def test_the_exact_form_differs_from_the_ordered_form_only_through_the_mean():
    """normalize = "exact" on a single domain: every output but net.S and the mean holds the bits of normalize = True, and net.S is
    the ordered run's net.S plus its mean minus the exact mean to rounding — the two means agree to the ordered sum's error bound."""
    rig = rig_with()
    try:
        outs = {}
        for normalize in (True, "exact"):
            outs[normalize] = out = tcs.Outputs(rig)
            sch, block = arguments(rig, out, backend=abi.HALO_NONE, normalize=normalize)
            rig.ctx.time_steps_coupled(0, STEPS, sch, rig.src, rig.w, out.fl, out.net, rig.stresses, block)
            rig.ctx.sync()
        ordered, exact = outs[True].bits(), outs["exact"].bits()
        for k in ordered:
            if k not in ("net.S", "mean"):
                assert torch.equal(ordered[k], exact[k]), k
        m1, m2 = float(outs[True].mean[0]), float(outs["exact"].mean[0])
        n = SHAPE[0] * SHAPE[1]
        # n terms summed in some order: |Δ| ≤ n · 2⁻⁵³ · Σ|t| / Σa, and Σ|t| / Σa ≤ max|v| (the areas are positive)
        bound = n * 2.0 ** -53 * float(torch.nan_to_num(outs["exact"].net["S"] + m2, nan=0.0).abs().max() + outs["exact"].restoring.nan_to_num(0.0).abs().max())
        assert m1 != 0.0 and abs(m1 - m2) <= bound, (m1, m2, bound)
    finally:
        rig.close()
