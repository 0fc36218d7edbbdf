"""The prescribed forcing components: JRA55PrescribedAtmosphere, JRA55PrescribedLand, Radiation and omip_forcing.  Both records
tell the time with clocks.RecordClock; their window back ends differ (pinned staging with a reader thread, a synchronous slot
table) and stay apart."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import abi, runtime, synthetic
from . import interface_computations as ic
from .clocks import RecordClock, hours


class JRA55PrescribedAtmosphere:
    """JRA55PrescribedAtmosphere(arch; dir, dataset, start_date, end_date, time_indices_in_memory,
    prefetch) — atmosphere.jl:20-29, README.md:74.  Holds `time_indices_in_memory` 3-hourly
    snapshots of the 9 variables (jra55_data_staging.jl:8) as Float32 640×320 fields in HBM.

    Two backends, as in the reference: everything in memory (`snapshots` = dict var -> [n, 320, 640]), or a
    sliding window (`provider(n) -> dict var -> [320, 640]` reads snapshot n from wherever the files are;
    `total_snapshots` per repeat-year/multi-year record).  With `prefetch` the snapshots the clock will reach next
    are read by a background thread straight into the window's pinned staging buffers and committed to HBM by the
    stepping thread, so file reads and PCIe copies overlap the flux kernels (launch.sh:86-93)."""

    def __init__(self, snapshots=None, *, provider=None, total_snapshots=None, time_indices_in_memory=2,
                 prefetch=True, time_interval=3 * hours, device=0, reference_height=10.0, boundary_layer_height=600.0,
                 cyclic=True, source_size=(synthetic.JRA55_NX, synthetic.JRA55_NY)):
        self.time_interval = time_interval
        self.reference_height = reference_height
        self.boundary_layer_height = boundary_layer_height
        self.cyclic = cyclic  # RepeatYearJRA55-style cyclic time indexing vs clamped (MultiYearJRA55 record ends)
        self.provider, self.prefetch = provider, prefetch
        self.window = None
        self._pending = {}   # time index -> Future of a background read into the pinned buffers
        self._reader = None
        if provider is not None:
            if total_snapshots is None:
                raise ValueError("a snapshot provider needs total_snapshots (2920 for a repeat year of 3-hourly JRA55)")
            if time_indices_in_memory < 2:
                raise ValueError("time_indices_in_memory must be >= 2")
            self.n_levels = total_snapshots
            self.n_slots = time_indices_in_memory
            self.source_size = source_size
            self.data = None
            return
        dev = torch.device("cuda", device)
        if snapshots is None:
            snapshots = synthetic.jra55_snapshots(time_indices_in_memory)
        self.data = {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in snapshots.items()}
        self.n_levels = next(iter(self.data.values())).shape[0]

    @property
    def record_clock(self):
        """The record clock (made on demand: n_levels, time_interval and cyclic are plain attributes that callers may set)."""
        return RecordClock(self.n_levels, self.time_interval, self.cyclic)

    def time_indices(self, t):
        """(n₁, n₂, ñ): the bracketing snapshots and the fractional position between them."""
        r = self.record_clock.at(t)
        return r.n1, r.n2, r.fraction

    # ---- sliding-window backend ---------------------------------------------------------------
    def _read_into_staging(self, k):
        """Snapshot COUNTER k (monotone in time, not wrapped) → the provider's record index wrap(k), staged in slot
        k mod n_slots.  Slots follow the counter, not the record index: at the end of a repeat year the indices
        jump from total−1 to 0, and two consecutive snapshots must never share a slot."""
        slot = k % self.n_slots
        self.window.wait_slot(slot)          # the previous copy out of these pinned buffers has finished
        snap = self.provider(self.record_clock.wrap(k))
        for v in abi.JRA55_VARIABLES:
            np.copyto(self.window.host_view(slot, v), snap[v], casting="same_kind")
        return slot

    def source(self, context, t):
        """The cf_atmos_source for time t.  In-memory backend: (data, n₁, n₂, ñ).  Window backend: makes n₁, n₂
        resident (blocking only if the prefetch has not delivered them), commits finished prefetches and queues
        the reads for the snapshots ahead."""
        base, k1, k2, n1, n2, frac = self.record_clock.at(t)
        if self.provider is None:
            return self.data, n1, n2, frac
        if self.window is None:
            self.window = runtime.SnapshotWindow(context, self.source_size[0], self.source_size[1], self.n_slots)
            if self.prefetch and self.n_slots > 2:
                from concurrent.futures import ThreadPoolExecutor
                self._reader = ThreadPoolExecutor(max_workers=1, thread_name_prefix="jra55-prefetch")
        w = self.window
        for k in (k1, k2):
            if w.find(k) >= 0:
                continue
            fut = self._pending.pop(k, None)
            slot = fut.result() if fut is not None else self._read_into_staging(k)
            w.commit(slot, k)
        for k, fut in list(self._pending.items()):      # prefetches that have landed in pinned memory
            if fut.done():
                w.commit(fut.result(), k)
                del self._pending[k]
        if self._reader is not None:
            for ahead in range(2, self.n_slots):        # the slots that hold neither k₁ nor k₂
                k = base + ahead
                if not self.cyclic and not (0 <= k < self.n_levels):
                    continue
                if k in (k1, k2) or w.find(k) >= 0 or k in self._pending:
                    continue
                if any((m % self.n_slots) == (k % self.n_slots) for m in list(self._pending) + [k1, k2]):
                    continue
                self._pending[k] = self._reader.submit(self._read_into_staging, k)
        return w.source(k1, k2, frac), n1, n2, frac

    def close(self):
        if self._reader is not None:
            self._reader.shutdown(wait=True)
            self._reader = None
        self._pending.clear()
        if self.window is not None:
            self.window.close()
            self.window = None


@dataclass
class Radiation:
    """JRA55PrescribedRadiation(arch; ocean_surface = SurfaceRadiationProperties(0.06, 1.00), …),
    atmosphere.jl:41-44 (the downwelling fields themselves ride in the atmosphere window)."""
    ocean_surface: ic.SurfaceRadiationProperties = field(default_factory=ic.SurfaceRadiationProperties)
    stefan_boltzmann_constant: float = 5.67e-8
    sea_ice_surface: Optional[ic.SurfaceRadiationProperties] = None   # SurfaceRadiationProperties(SeaIceAlbedo(hi, hs, Ts), 1.0)


JRA55PrescribedRadiation = Radiation


class JRA55PrescribedLand:
    """JRA55PrescribedLand(arch; …) — atmosphere.jl:46: river discharge and calving (friver, licalvf of
    jra55_data_staging.jl:8) as 3-hourly Float32 windows on the JRA55 grid; OceanSeaIceModel(…; land) interpolates them
    each step and the freshwater reaches the salinity flux.

    Two backends, like the atmosphere: the whole record in memory (`snapshots` = {friver, licalvf}: [n, 320, 640]), or a
    sliding window of `time_indices_in_memory` device slots fed by `provider(n) -> {friver, licalvf}: [320, 640]`
    (`total_snapshots` records; `cyclic` = RepeatYearJRA55, clamped = MultiYearJRA55).  The window follows the monotone
    snapshot COUNTER (slot = counter mod slots), so a repeat year whose length is no multiple of the slot count never
    puts two consecutive snapshots in one slot.  Two 0.8 MB planes per 3 h: read synchronously, no prefetch thread."""

    def __init__(self, snapshots=None, *, provider=None, total_snapshots=None, time_indices_in_memory=2, time_interval=3 * hours,
                 device=0, cyclic=True, source_size=(synthetic.JRA55_NX, synthetic.JRA55_NY)):
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.time_interval = time_interval
        self.cyclic = cyclic
        self.provider = provider
        if provider is not None:
            if total_snapshots is None:
                raise ValueError("a snapshot provider needs total_snapshots")
            if time_indices_in_memory < 2:
                raise ValueError("time_indices_in_memory must be >= 2")
            self.n_levels = total_snapshots
            self.n_slots = time_indices_in_memory
            shape = (self.n_slots, source_size[1], source_size[0])
            self.data = {k: torch.zeros(shape, dtype=torch.float32, device=dev) for k in ("friver", "licalvf")}
            self._slot_counter = [None] * self.n_slots   # which snapshot counter each slot holds
            return
        if snapshots is None:
            snapshots = synthetic.jra55_land_snapshots(time_indices_in_memory)
        self.data = {k: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in snapshots.items()}
        self.n_levels = self.data["friver"].shape[0]

    @property
    def record_clock(self):
        return RecordClock(self.n_levels, self.time_interval, self.cyclic)

    def levels(self, t):
        """(level1, level2, ñ) into `self.data` for model time t — the bracketing snapshots made resident first on the
        sliding-window backend.  Cyclic (repeat year) or clamped (multi-year record ends) like the atmosphere."""
        clock = self.record_clock
        _, k1, k2, n1, n2, frac = clock.at(t)
        if self.provider is None:
            return n1, n2, frac
        for k in (k1, k2):
            slot = k % self.n_slots
            if self._slot_counter[slot] != k:
                snap = self.provider(clock.wrap(k))
                for v, dst in self.data.items():
                    plane = snap.get(v)
                    if plane is None:
                        dst[slot].zero_()
                    else:
                        dst[slot].copy_(torch.from_numpy(np.array(plane, dtype=np.float32)))  # (a copy: memory-mapped planes are read-only)
                self._slot_counter[slot] = k
        return k1 % self.n_slots, k2 % self.n_slots, frac


def omip_forcing(arch, sea_ice, *, forcing_dir, start_date, end_date, repeat_year_forcing=False, backend_size=30, device=0):
    """omip_forcing(arch, sea_ice; forcing_dir, start_date, end_date, repeat_year_forcing = false, backend_size = 30)
    — /root/reference/src/OMIPConfigurations/atmosphere.jl:13-49: the prescribed forcing components of an OMIP-2
    simulation.  Returns `(atmosphere, radiation, land)`: the JRA55-do atmosphere on a sliding window of `backend_size`
    snapshots with prefetch, the downwelling radiation with the OMIP-2 ocean surface (albedo 0.06, emissivity 1) and
    the CCSM3 `SeaIceAlbedo(hi, hs, Ts)` over ice, and the land freshwater (river runoff + iceberg calving).
    `arch` is accepted for signature parity (the device is `device`).  Files: raw Float32 planes, see coflux/jra55.py."""
    from . import jra55
    dataset = jra55.RepeatYearJRA55(year=start_date.year) if repeat_year_forcing else jra55.MultiYearJRA55()
    calendar = jra55.SnapshotCalendar(dataset, start_date, end_date)
    files = jra55.RawPlaneFiles(forcing_dir)
    atmosphere = JRA55PrescribedAtmosphere(provider=jra55.atmosphere_provider(forcing_dir, calendar, files), total_snapshots=calendar.total,
                                           time_indices_in_memory=backend_size, prefetch=True, cyclic=dataset.cyclic, device=device)
    atmosphere.dataset, atmosphere.calendar = dataset, calendar
    sea_ice_albedo = ic.SeaIceAlbedo() if sea_ice is not None else None   # SeaIceAlbedo(hi, hs, Ts): reads the live ice fields
    radiation = Radiation(ocean_surface=ic.SurfaceRadiationProperties(0.06, 1.00),
                          sea_ice_surface=ic.SurfaceRadiationProperties(sea_ice_albedo, 1.0) if sea_ice is not None else None)
    # JRA55PrescribedLand(arch; …) streams the whole record like the atmosphere: same calendar, same window length
    land = JRA55PrescribedLand(provider=jra55.land_provider(forcing_dir, calendar, files), total_snapshots=calendar.total,
                               time_indices_in_memory=max(2, backend_size), cyclic=dataset.cyclic, device=device)
    land.dataset, land.calendar = dataset, calendar
    return atmosphere, radiation, land
