"""models.ExchangeStates — the owner of the two exchange field sets behind interfaces.exchange_atmosphere_state and of the
request-ahead state of run!(simulation) — against a recording stand-in for the context.  The expected call sequences are
written out from the code the owner replaced: update_state! swapped the sets when the previous step had requested a state,
then (with a stepping Δt) made the other set on first use, set CF_OPT_MERGED_PREFETCH = 2 once, asked the atmosphere for the
source at t + Δt and called prefetch_atmosphere_state into the other set, then launched the solver on the current set; the
exit of run! dropped the request, called discard_prefetched_atmosphere_state, copied set 1 into set 0 if set 1 was current,
and set the option back to 0 if it had been set."""
from types import SimpleNamespace

from coflux import abi
from coflux import models as cm
from coflux.runtime import EXCHANGE_NAMES

DT = 1200.0


class Field:
    def __init__(self, log, name, value=0.0):
        self.log, self.name, self.value = log, name, value

    def copy_(self, other):
        self.log.append(("copy", self.name, other.name))
        self.value = other.value


class Context:
    """records every call the owner makes, in order"""

    def __init__(self):
        self.log, self.sets_made = [], 0

    def field_set(self, names):
        self.sets_made += 1
        self.log.append(("field_set", tuple(names)))
        return {k: Field(self.log, f"made{self.sets_made}.{k}") for k in names}

    def set_option(self, option, value):
        self.log.append(("set_option", option, value))

    def prefetch_atmosphere_state(self, src, weights, atmos_next, level1=0, level2=1, time_fraction=0.0):
        self.log.append(("prefetch", src, weights, id(atmos_next), level1, level2, time_fraction))

    def discard_prefetched_atmosphere_state(self):
        self.log.append(("discard",))


def scenario(nsteps):
    """`nsteps` steps as update_state! takes them under run!(simulation), each writing its number into the current set as the
    solver launch does; returns the owner, the context, both sets' identities as they are after the steps, and which set was
    current at each step"""
    ctx = Context()
    stable = {k: Field(ctx.log, f"stable.{k}") for k in EXCHANGE_NAMES}
    ex = cm.ExchangeStates(ctx, stable)
    assert ex.stable is stable and ex.current is stable and ex.other is None and not ex.inside_run and ex.stepping_dt is None
    atmosphere = SimpleNamespace(source=lambda context, t: (ctx.log.append(("source", t)) or "src", int(t // 10800) % 4, int(t // 10800 + 1) % 4,
                                                             t / 10800 - t // 10800))
    ex.stepping_dt = DT
    assert ex.inside_run
    currents, t = [], 0.0
    for step in range(1, nsteps + 1):
        t += DT
        ex.begin_step()
        ex.request_next(atmosphere, "weights", t + ex.stepping_dt)
        assert ex.inside_run
        currents.append(0 if ex.current is stable else 1)
        ctx.log.append(("update_state", id(ex.current)))
        for f in ex.current.values():
            f.value = float(step)
    return ex, ctx, stable, currents


def expected_steps(nsteps, stable, other):
    """the parent's sequence for the same steps"""
    want, sets = [], (stable, other)
    for step in range(1, nsteps + 1):
        current = (step - 1) % 2
        if step == 1:
            want += [("field_set", tuple(EXCHANGE_NAMES)), ("set_option", abi.OPT_MERGED_PREFETCH, 2)]
        t = (step + 1) * DT
        want += [("source", t), ("prefetch", "src", "weights", id(sets[1 - current]), int(t // 10800) % 4, int(t // 10800 + 1) % 4, t / 10800 - t // 10800),
                 ("update_state", id(sets[current]))]
    return want


def test_three_steps_and_the_way_out_of_run():
    ex, ctx, stable, currents = scenario(3)
    assert currents == [0, 1, 0], "the current set alternates"
    assert ctx.sets_made == 1 and ex.other is not None and ex.other is not stable, "the other set is made once"
    other = ex.other
    assert [c for c in ctx.log if c[0] == "set_option"] == [("set_option", abi.OPT_MERGED_PREFETCH, 2)]
    assert ctx.log == expected_steps(3, stable, other)
    held = {k: f.value for k, f in ex.current.items()}
    assert set(held.values()) == {3.0}
    del ctx.log[:]
    ex.settle()
    # current == 0: nothing is copied; the request is dropped here and in the library; the option goes back, once
    assert ctx.log == [("discard",), ("set_option", abi.OPT_MERGED_PREFETCH, 0)]
    assert ex.current is stable and ex.stable is stable and {k: f.value for k, f in stable.items()} == held
    assert not ex.inside_run and ex.stepping_dt is None
    # a second settle: the discard call that run! makes on every exit, and nothing else
    del ctx.log[:]
    ex.settle()
    assert ctx.log == [("discard",)] and ex.current is stable
    # … and a step taken by hand afterwards does not mistake the state run! had requested ahead for its own
    ex.begin_step()
    assert ex.current is stable and ctx.log == [("discard",)]


def test_settling_on_the_other_set_brings_the_state_back_to_set_0():
    ex, ctx, stable, currents = scenario(2)
    assert currents == [0, 1]
    other = ex.current                   # the set made by the first request: the second step's state is in it
    assert ex.other is stable
    assert ctx.log == expected_steps(2, stable, other)
    assert ex.current is other and {f.value for f in other.values()} == {2.0} and {f.value for f in stable.values()} == {1.0}
    del ctx.log[:]
    ex.settle()
    want = [("discard",)] + [("copy", f"stable.{k}", f"made1.{k}") for k in EXCHANGE_NAMES] + [("set_option", abi.OPT_MERGED_PREFETCH, 0)]
    assert ctx.log == want
    assert ex.current is stable and all(f.value == 2.0 for f in stable.values()) and not ex.inside_run
    assert ctx.sets_made == 1


def test_a_pending_request_is_dropped_by_settle_and_by_a_pickup():
    ex, ctx, stable, _ = scenario(1)
    assert ex.inside_run and ex.current is stable
    del ctx.log[:]
    ex.settle()                          # the requested state of a step that will not run
    assert ctx.log == [("discard",), ("set_option", abi.OPT_MERGED_PREFETCH, 0)]
    ex.begin_step()
    assert ex.current is stable, "the dropped request is not swapped in"
    # Checkpointer.pickup: drop_request, then set 0 ← the checkpoint's exchange fields; the option is not touched
    ex, ctx, stable, _ = scenario(2)
    image = {k: Field(ctx.log, f"image.{k}", 42.0) for k in EXCHANGE_NAMES}
    del ctx.log[:]
    ex.drop_request()
    ex.restore(image)
    assert ctx.log == [("discard",)] + [("copy", f"stable.{k}", f"image.{k}") for k in EXCHANGE_NAMES]
    assert ex.current is stable and all(f.value == 42.0 for f in stable.values())
    ex.begin_step()
    assert ex.current is stable


def test_without_a_stepping_dt_nothing_is_requested():
    ctx = Context()
    ex = cm.ExchangeStates(ctx, {"Ta": Field(ctx.log, "stable.Ta")})
    for _ in range(3):                   # time_step! in a plain loop: update_state! asks for nothing
        ex.begin_step()
    assert ctx.log == [] and ex.other is None and not ex.inside_run and ctx.sets_made == 0
