"""Checkpointer: the output writer behind run!(simulation; pickup) — packed device snapshots of cf_checkpoint_*."""
import json
import os
import re
import warnings

import numpy as np
import torch

from .clocks import days
from .outputs import MonthlyClimatology, SurfaceFluxAverages, _SeriesWriter
from .runtime import EXCHANGE_NAMES, checkpoint_host_blob
from .schedules import AveragedTimeInterval, TimeInterval, actuates, as_schedule, open_at


# ---------------------------------------------------------------------------------------------
# checkpoint and pickup (cf_checkpoint_*): Checkpointer, run!(simulation; pickup = true)
# ---------------------------------------------------------------------------------------------
class Checkpointer:
    """Checkpointer(model; schedule = TimeInterval(…) | IterationInterval(n), dir = ".", prefix = "checkpoint", cleanup =
    false) — the output writer every reference launch installs (omip_diagnostics.jl:220-225), for run!(simulation; pickup).
    The files `<dir>/<prefix>_iteration<N>.cfck` are images of cf_checkpoint_capture: THIS LIBRARY'S OWN FORMAT, NOT JLD2.
    initialize(simulation) registers every device field of the model — the ocean's T, S, u, v (whole 3-D arrays), wet_mask, the
    top boundary condition fields and the shortwave flux, every sea-ice field that is set, the exchange state at the model's
    clock (through a staging set of the writer's: inside run! the current state alternates between two sets), the interface
    and net-flux fields, land_freshwater, the ice–ocean fluxes, and the buffers of a NormalizeSalinity among the callbacks —
    and, of every SurfaceFluxAverages, MonthlyClimatology, SurfaceIntegrals and SurfaceExtrema among the simulation's writers,
    the device arrays and the library handles (weights, counts, times, records, the monitor's status).  The image's host blob
    is JSON: both clocks, each writer's schedule state (AveragedTimeInterval.k / .previous, the climatology's window), the
    registered names.
    write() captures — stream ordered, one launch — and returns; the image drains while the next steps run, and the file is
    written (to a temporary name, then renamed; `cleanup` then removes the previous file — after a pickup that is the file
    picked up, once the next one is whole) by the next write(), by flush() or by close().
    NOT in a checkpoint: what a writer has already delivered to the host — SurfaceFluxAverages.windows, the drained chunks of
    a series writer (`_values`, `_times`) — which is the caller's, as the reference's output files are; the
    atmosphere and land windows, which are re-read for the restored clock; the solver's schedules and hints, which are rebuilt
    and never change a bit."""
    SUFFIX = ".cfck"

    def __init__(self, model, schedule=None, dir=".", prefix="checkpoint", cleanup=False, direct=False):
        self.model = model
        self.schedule = as_schedule(schedule, TimeInterval(30 * days))
        self.dir, self.prefix, self.cleanup, self.direct = str(dir), str(prefix), bool(cleanup), bool(direct)
        self.checkpoint = None      # the runtime.Checkpoint, made by initialize
        self.names = []
        self._simulation = None
        self._pending = None        # iteration of the capture whose image is still draining
        self._previous_file = None
        self._exchange = None

    # -- files ------------------------------------------------------------------------------------
    def path(self, iteration):
        return os.path.join(self.dir, f"{self.prefix}_iteration{int(iteration)}{self.SUFFIX}")

    def iterations(self):
        """The iterations of this writer's files in `dir`, ascending."""
        pattern = re.compile(re.escape(self.prefix) + r"_iteration(\d+)" + re.escape(self.SUFFIX) + "$")
        found = [pattern.match(name) for name in (os.listdir(self.dir) if os.path.isdir(self.dir) else [])]
        return sorted(int(m.group(1)) for m in found if m)

    def latest(self):
        """The path of the file with the highest iteration, or None."""
        its = self.iterations()
        return self.path(its[-1]) if its else None

    def _write_file(self, iteration, image):
        os.makedirs(self.dir, exist_ok=True)
        path = self.path(iteration)
        tmp = path + ".tmp"
        with open(tmp, "wb") as f:
            f.write(image)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)   # a reader finds the old file or the whole new one, never a part
        if self.cleanup and self._previous_file and self._previous_file != path and os.path.exists(self._previous_file):
            os.remove(self._previous_file)
        self._previous_file = path

    # -- registration -----------------------------------------------------------------------------
    def _add(self, name, tensor):
        """Registers `tensor` unless its bytes are already part of a registered array (the top boundary conditions ARE the net
        fluxes, the sea ice's interface_heat IS the ice–ocean exchange's)."""
        if tensor is None or not isinstance(tensor, torch.Tensor):
            return
        lo, hi = tensor.data_ptr(), tensor.data_ptr() + tensor.numel() * tensor.element_size()
        if any(a <= lo and hi <= b for a, b in self._ranges):
            return
        self.checkpoint.add_array(name, tensor)
        self._ranges.append((lo, hi))
        self.names.append(name)

    def initialize(self, simulation):
        if self.checkpoint is not None:
            open_at(self.schedule, self.model.clock.time, simulation.dt)
            return
        self._simulation = simulation
        m, itf = self.model, self.model.interfaces
        ctx = itf.context
        self.checkpoint = ctx.checkpoint(direct=self.direct)
        self._ranges, self.names = [], []
        om = m.ocean.model
        for name, t in (("ocean.T", om.tracers.T), ("ocean.S", om.tracers.S), ("ocean.u", om.velocities.u), ("ocean.v", om.velocities.v),
                        ("ocean.wet_mask", om.wet_mask), ("ocean.shortwave_surface_flux", om.shortwave_surface_flux)):
            self._add(name, t)
        for k in ("u", "v", "T", "S"):
            bc = getattr(om.top_boundary_conditions, k)
            self._add(f"ocean.top.{k}", getattr(bc, "flux_field", bc))   # (of a MultipleFluxes; a bare field is its own)
        if m.sea_ice is not None:
            for k in ("concentration", "interface_heat", "salt_flux", "x_stress", "y_stress", "thickness", "top_surface_temperature", "u", "v",
                      "albedo", "frazil_heat", "snow_thickness"):
                self._add(f"sea_ice.{k}", getattr(m.sea_ice, k))
        self._exchange = ctx.field_set(EXCHANGE_NAMES)
        for k, t in self._exchange.items():
            self._add(f"exchange.{k}", t)
        groups = [("atmosphere_ocean", itf.atmosphere_ocean_interface._fields), ("net.ocean", itf.net_fluxes._ocean_fields)]
        if itf.atmosphere_sea_ice_interface is not None:
            groups += [("atmosphere_sea_ice", itf.atmosphere_sea_ice_interface._fields), ("net.sea_ice", itf.net_fluxes._sea_ice_fields)]
        if getattr(itf, "sea_ice_ocean_heat_flux", None) is not None:
            groups.append(("sea_ice_ocean", itf.sea_ice_ocean_fluxes))
        for group, fields in groups:
            for k, t in fields.items():
                self._add(f"{group}.{k}", t)
        self._add("land_freshwater", itf.land_freshwater)
        for cname, cb in simulation.callbacks.items():   # a callback with device state of its own (NormalizeSalinity) names it
            for k, t in getattr(cb.func, "checkpoint_arrays", dict)().items():
                self._add(f"callback.{cname}.{k}", t)
        for wname, w in simulation.output_writers.items():
            if isinstance(w, SurfaceFluxAverages):
                for k, t in w.means.items():
                    self._add(f"{wname}.mean.{k}", t)
                for k, t in (w._budget_atmos or {}).items():
                    self._add(f"{wname}.budget.{k}", t)
                for n, a in enumerate(w.averagers):
                    self._add_handle(f"{wname}.averager{n}", a)
            elif isinstance(w, MonthlyClimatology):
                for k in w.names:
                    self._add(f"{wname}.total.{k}", w.totals[k])
                    self._add(f"{wname}.bins.{k}", w.bins[k])
                self._add_handle(f"{wname}.climatology", w.climatology)
            elif isinstance(w, _SeriesWriter):
                self._add_handle(f"{wname}.series", w._recorder)
        too_long = [n for n in self.names if len(n.encode()) > 47]
        assert not too_long, too_long
        open_at(self.schedule, m.clock.time, simulation.dt)

    def _add_handle(self, name, handle):
        self.checkpoint.add(name, handle)
        self.names.append(name)

    # -- the host blob ----------------------------------------------------------------------------
    def _state(self):
        """What the image's host blob holds (JSON): both clocks, every writer's schedule state, the registered names."""
        m = self.model
        writers = {}
        for wname, w in (self._simulation.output_writers.items() if self._simulation is not None else ()):
            s = getattr(w, "schedule", None)
            if isinstance(s, AveragedTimeInterval):
                writers[wname] = dict(kind="averaged", k=s.k, previous=s.previous)
            elif isinstance(w, MonthlyClimatology):
                writers[wname] = dict(kind="climatology", start_time=w.start_time, stop_time=w.stop_time, reference_date=w.reference_date.isoformat())
        return dict(format="coflux-checkpoint", clock=dict(time=m.clock.time, iteration=m.clock.iteration),
                    ocean_clock=dict(time=m.ocean.model.clock.time, iteration=m.ocean.model.clock.iteration), writers=writers,
                    names=list(self.names))

    def _check_state(self, state, path):
        """ValueError unless the blob is this simulation's: the same registration, the same writers, the same climatology window."""
        if state.get("names") != list(self.names):
            raise ValueError(f"pickup: {path} was written by another registration than this simulation's")
        for wname, s in state["writers"].items():
            w = self._simulation.output_writers.get(wname)
            if w is None:
                raise ValueError(f"pickup: {path} has the state of a writer {wname!r} that this simulation lacks")
            if s["kind"] == "climatology" and (s["start_time"], s["stop_time"]) != (w.start_time, w.stop_time):
                raise ValueError(f"pickup: the climatology {wname!r} of {path} was collected over another window")

    def _set_state(self, state):
        m = self.model
        m.clock.time, m.clock.iteration = float(state["clock"]["time"]), int(state["clock"]["iteration"])
        m.ocean.model.clock.time, m.ocean.model.clock.iteration = float(state["ocean_clock"]["time"]), int(state["ocean_clock"]["iteration"])
        for wname, s in state["writers"].items():
            if s["kind"] == "averaged":
                w = self._simulation.output_writers[wname]
                w.schedule.k, w.schedule.previous = int(s["k"]), float(s["previous"])

    # -- the writer -------------------------------------------------------------------------------
    def write(self, clock):
        self.flush()
        if not actuates(self.schedule, clock):
            return
        if self._exchange is not None:   # the exchange state at the model's clock, wherever run! keeps it at this step
            current = self.model.interfaces.exchange_atmosphere_state
            for k, t in self._exchange.items():
                t.copy_(current[k])
        self.checkpoint.set_host_blob(json.dumps(self._state()).encode())
        self.checkpoint.capture()
        self._pending = int(clock.iteration)

    def flush(self):
        """Waits for the image of the last capture, if one is still draining, and writes its file."""
        if self._pending is None:
            return
        iteration, self._pending = self._pending, None
        self._write_file(iteration, self.checkpoint.wait(copy=False))

    def close(self):
        self.flush()
        if self.checkpoint is not None:
            self.checkpoint.close()

    # -- pickup -----------------------------------------------------------------------------------
    def pickup(self, which=True):
        """Restores the model, the other writers and the clocks from a file: True / "latest" the highest iteration (None found:
        a warning, nothing restored, returns None), an int that iteration, any other str that path.  Returns the path."""
        if which is True or which == "latest":
            path = self.latest()
            if path is None:
                warnings.warn(f"pickup: no {self.prefix}_iteration*{self.SUFFIX} in {self.dir!r}; starting from scratch")
                return None
        else:
            path = self.path(which) if isinstance(which, (int, np.integer)) else str(which)
            if not os.path.exists(path):
                raise FileNotFoundError(f"pickup: {path} does not exist")
        with open(path, "rb") as f:
            image = f.read()
        state = json.loads(checkpoint_host_blob(image).decode())   # (verifies the whole image first)
        self._check_state(state, path)                             # nothing is restored from a file of another simulation
        self.checkpoint.restore(image)
        self._set_state(state)
        itf = self.model.interfaces
        # the state at the model's clock lies in exchange set 0, nothing is requested ahead: what run!'s own exit establishes
        itf.exchange.drop_request()
        itf.exchange.restore(self._exchange)
        if getattr(self.model, "land", None) is not None and itf.land_freshwater is not None:
            itf.context.set_land_freshwater(itf.land_freshwater)
        if self._simulation is not None:
            open_at(self.schedule, self.model.clock.time, self._simulation.dt)
        itf.context.sync()   # the restore's device-side hashes are checked here
        self._previous_file = path
        return path
