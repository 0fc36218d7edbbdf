"""AveragedTimeInterval bookkeeping (coflux.models) against hand-computed tables, and the output-writer protocol of run! —
no GPU: the schedule is host arithmetic, and SurfaceFluxAverages is driven here through a stand-in context whose averager
restates cf_average_collect on the CPU.

Window k is (t_k − window, t_k] with t_k = k · interval; a step's sample is taken when iteration % stride == 0 and always at
t_k, with weight t_n − max(t_prev_sample, t_k − window)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from coflux import models as cm


def table(schedule, steps, dt=1.0, t0=0.0, it0=0):
    """[(iteration, weight, t_k)] of every step that collects"""
    schedule.initialize(t0, dt)
    out = []
    for n in range(1, steps + 1):
        w, t_k = schedule.sample(t0 + n * dt, it0 + n)
        if w is not None:
            out.append((it0 + n, w, t_k))
        else:
            assert t_k is None
    return out


def test_every_step_window_equals_interval():
    assert table(cm.AveragedTimeInterval(4.0), 8) == [(1, 1.0, None), (2, 1.0, None), (3, 1.0, None), (4, 1.0, 4.0),
                                                       (5, 1.0, None), (6, 1.0, None), (7, 1.0, None), (8, 1.0, 8.0)]


def test_window_shorter_than_interval_with_stride():
    # windows (1, 4], (5, 8], (9, 12]; stride 2 samples iterations 2, 6, 10 and the forced ends 4, 8, 12
    assert table(cm.AveragedTimeInterval(4.0, window=3.0, stride=2), 12) == [
        (2, 1.0, None), (4, 2.0, 4.0), (6, 1.0, None), (8, 2.0, 8.0), (10, 1.0, None), (12, 2.0, 12.0)]


def test_stride_sample_before_the_window_opens_is_not_taken():
    # windows (6, 10], (16, 20]; stride 3: 3 and 6 (the open edge) are outside, 9 → 9 − 6, 10 forced → 1; 12, 15 outside,
    # 18 → 18 − 16, 20 forced (20 % 3 ≠ 0) → 2
    assert table(cm.AveragedTimeInterval(10.0, window=4.0, stride=3), 20) == [
        (9, 3.0, None), (10, 1.0, 10.0), (18, 2.0, None), (20, 2.0, 20.0)]


def test_stride_longer_than_the_gap_to_the_window_end():
    # interval 6, stride 4: 4 → 4, 6 forced → 2 (since the sample at 4), 8 → 2, 12 (forced and on the stride) → 4
    assert table(cm.AveragedTimeInterval(6.0, stride=4), 12) == [(4, 4.0, None), (6, 2.0, 6.0), (8, 2.0, None), (12, 4.0, 12.0)]


def test_start_inside_a_window_weights_from_the_start():
    # the run starts at t = 5 (iteration 5): the open window (4, 8] is weighted from the start of the run
    assert table(cm.AveragedTimeInterval(4.0), 4, t0=5.0, it0=5) == [(6, 1.0, None), (7, 1.0, None), (8, 1.0, 8.0), (9, 1.0, None)]


def test_open_window_survives_a_second_run():
    s = cm.AveragedTimeInterval(4.0)
    s.initialize(0.0, 1.0)
    assert [s.sample(float(n), n) for n in (1, 2)] == [(1.0, None), (1.0, None)]
    s.initialize(2.0, 1.0)                      # run! again: the window (0, 4] stays open
    assert [s.sample(float(n), n) for n in (3, 4)] == [(1.0, None), (1.0, 4.0)]


def test_omip_five_day_means_at_twenty_minutes():
    rows = table(cm.AveragedTimeInterval(5 * cm.days), 2 * 360, dt=20 * cm.minutes)
    assert len(rows) == 720 and all(w == 1200.0 for _, w, _ in rows)
    assert [(n, t_k) for n, _, t_k in rows if t_k is not None] == [(360, 432000.0), (720, 864000.0)]


@pytest.mark.parametrize("interval, window, stride", [(12.0, 12.0, 5), (12.0, 7.0, 5), (12.0, 2.5, 1), (30.0, 11.0, 7)])
def test_weights_of_a_window_add_up_to_the_window(interval, window, stride):
    rows = table(cm.AveragedTimeInterval(interval, window=window, stride=stride), 120)
    ends = [n for n, _, t_k in rows if t_k is not None]
    assert ends == [int(k * interval) for k in range(1, len(ends) + 1)] and len(ends) == int(120 // interval)
    total = 0.0
    for _, w, t_k in rows:
        assert w > 0
        total += w
        if t_k is not None:
            assert total == pytest.approx(window, abs=1e-12)
            total = 0.0


def test_rejects_a_time_step_that_does_not_divide_the_interval():
    with pytest.raises(ValueError, match="does not divide"):
        cm.AveragedTimeInterval(5 * cm.days).initialize(0.0, 7 * cm.minutes)
    with pytest.raises(ValueError, match="does not divide"):
        cm.AveragedTimeInterval(10.0).initialize(0.0, 20.0)
    with pytest.raises(ValueError, match="does not divide"):
        cm.AveragedTimeInterval(10.0).initialize(0.0, 0.0)
    cm.AveragedTimeInterval(1.0).initialize(0.0, 0.1)       # 10 steps of 0.1: divides up to rounding
    for bad in (dict(interval=0.0), dict(interval=4.0, window=5.0), dict(interval=4.0, window=0.0), dict(interval=4.0, stride=0),
                dict(interval=4.0, stride=1.5)):
        with pytest.raises(ValueError):
            cm.AveragedTimeInterval(**bad)


# ---- the writer and run!, on a stand-in context ---------------------------------------------------------------------------
class _Averager:
    """cf_average_collect restated on the CPU (the kernel's recurrence on the whole array)"""

    def __init__(self, sources, means):
        self.sources, self.means, self.total, self.samples = sources, means, 0.0, 0

    def collect(self, w):
        total = self.total + w
        for f, m in zip(self.sources, self.means):
            m.copy_(f if self.samples == 0 else m * (self.total / total) + f * (w / total))
        self.total, self.samples = total, self.samples + 1

    def reset(self):
        self.total, self.samples = 0.0, 0


def _fake_model(nx=5, ny=3, h=1):
    shape = (ny + 2 * h, nx + 2 * h)
    ctx = SimpleNamespace(zeros=lambda: torch.zeros(shape, dtype=torch.float64), average=_Averager,
                          discard_prefetched_atmosphere_state=lambda: None, sync=lambda: None)
    net = {k: torch.zeros(shape, dtype=torch.float64) for k in ("u", "v", "T", "S")}
    ao = {k: torch.zeros(shape, dtype=torch.float64) for k in ("sensible_heat", "latent_heat")}
    itf = SimpleNamespace(context=ctx, net_fluxes=SimpleNamespace(_ocean_fields=net), atmosphere_ocean_interface=SimpleNamespace(_fields=ao),
                          _exchange_current=0)
    grid = SimpleNamespace(size=(nx, ny, 1), halo=(h, h, 1))
    return SimpleNamespace(interfaces=itf, ocean=SimpleNamespace(grid=grid), clock=SimpleNamespace(time=0.0, iteration=0)), net, ao


def test_run_hands_every_writer_the_clock_and_surface_averages_close_their_windows(monkeypatch):
    model, net, ao = _fake_model()

    def fake_step(m, dt):           # every field takes the value of the step's iteration
        m.clock.time += dt
        m.clock.iteration += 1
        for t in list(net.values()) + list(ao.values()):
            t.fill_(float(m.clock.iteration))

    monkeypatch.setattr(cm, "time_step", fake_step)
    seen = []
    writer = cm.SurfaceFluxAverages(model, schedule=cm.AveragedTimeInterval(4.0, window=3.0, stride=2),
                                    on_window=lambda t_k, arrays: seen.append(t_k))
    assert set(writer.outputs) == {"tauuo", "tauvo", "hfds", "wfo", "hfss", "hfls"}
    assert writer.outputs["hfds"] is net["T"] and writer.outputs["hfls"] is ao["latent_heat"]
    clocks = []
    log = SimpleNamespace(initialize=lambda sim: clocks.append("init"), write=lambda clock: clocks.append(clock.iteration))
    sim = cm.Simulation(model, dt=1.0, stop_iteration=9, output_writers={"surface": writer, "log": log})
    assert cm.Simulation(model).output_writers == {}
    cm.run(sim)
    assert clocks == ["init"] + list(range(1, 10))
    # windows (1, 4] and (5, 8]: samples 2 (weight 1) and 4 (weight 2), then 6 (1) and 8 (2); 9 is outside every window
    assert seen == [4.0, 8.0] and [t for t, _ in writer.windows] == [4.0, 8.0]
    for (t_k, arrays), want in zip(writer.windows, ((2 * 1 + 4 * 2) / 3, (6 * 1 + 8 * 2) / 3)):
        assert set(arrays) == set(writer.outputs)
        for a in arrays.values():
            assert a.shape == (3, 5) and np.allclose(a, want, rtol=1e-15)
    # the open window survives the end of run!: 10 is its first sample
    sim.stop_iteration = 10
    cm.run(sim)
    assert writer.averager.samples == 1 and writer.averager.total == 1.0 and len(writer.windows) == 2


def test_a_writer_refuses_a_time_step_that_does_not_divide_its_interval(monkeypatch):
    model, _, _ = _fake_model()
    monkeypatch.setattr(cm, "time_step", lambda m, dt: pytest.fail("no step may run"))
    writer = cm.SurfaceFluxAverages(model, schedule=cm.AveragedTimeInterval(5 * cm.days))
    with pytest.raises(ValueError, match="does not divide"):
        cm.run(cm.Simulation(model, dt=7 * cm.minutes, stop_iteration=3, output_writers={"surface": writer}))
