"""Thin runtime over the C ABI: a FluxContext owns one cf_ctx (one GPU), fields are torch CUDA
tensors used purely as device-memory plumbing (their data_ptr() goes through the ABI).

There is no CPU compute path here.  Creating a FluxContext without a GPU / without
libcoflux.so raises.
"""
import ctypes as C

import numpy as np
import torch

from . import abi

EXCHANGE_NAMES = ("u", "v", "T", "p", "q", "Qs", "Ql", "Mp")
FLUX_NAMES = ("sensible_heat", "latent_heat", "water_vapor", "x_momentum", "y_momentum", "temperature")
FLUX_OPTIONAL = ("friction_velocity", "temperature_scale", "humidity_scale")
NET_NAMES = ("u", "v", "T", "S", "shortwave_surface_flux", "upwelling_longwave",
             "downwelling_longwave", "downwelling_shortwave")
ICE_NAMES = ("concentration", "interface_heat", "salt_flux", "x_stress", "y_stress")


class CofluxError(RuntimeError):
    pass


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _is_field(t, ctx, dtype=torch.float64):
    """A contiguous device array of the context's shape and of `dtype` (None: any): what every ocean-grid array handed to
    the library is."""
    return t.is_cuda and t.is_contiguous() and tuple(t.shape) == ctx.shape and dtype in (None, t.dtype)


class FluxContext:
    """One libcoflux context bound to `device` (cuda:N)."""

    def __init__(self, nx, ny, hx, hy, params, ring=1, device=0):
        self.lib = abi.load_library()
        if not torch.cuda.is_available():
            raise CofluxError("coflux needs a HIP device (torch.cuda.is_available() is False); "
                              "there is no CPU compute path")
        self.device = torch.device("cuda", device)
        self.grid = abi.Grid(nx, ny, hx, hy, ring, 0)
        self.params = params
        self.shape = (ny + 2 * hy, nx + 2 * hx)
        self._h = C.c_void_p()
        rc = self.lib.cf_create(C.byref(self._h), device, C.byref(self.grid), C.byref(params))
        if rc != 0:
            raise CofluxError(f"cf_create failed ({rc}): {self.lib.cf_last_error(None).decode()}")
        self.use_torch_stream()

    # -- lifecycle ----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.cf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise CofluxError(f"{what} failed ({rc}): {self.lib.cf_last_error(self._h).decode()}")

    def use_torch_stream(self):
        """Order libcoflux launches on torch's current stream for this device."""
        s = torch.cuda.current_stream(self.device).cuda_stream
        # torch's default stream has handle 0 = the legacy null stream; 0 means "own stream" in the ABI
        self._check(self.lib.cf_set_stream(self._h, C.c_void_p(s if s else 1)), "cf_set_stream")

    def set_flux_params(self, params):
        self._check(self.lib.cf_set_flux_params(self._h, C.byref(params)), "cf_set_flux_params")
        self.params = params

    def set_option(self, option, value):
        self._check(self.lib.cf_set_option(self._h, option, value), "cf_set_option")

    def debug_eval(self, function, x):
        """y = f(x) with the device primitives of the solver (self-test hook)."""
        y = torch.empty_like(x)
        self._check(self.lib.cf_debug_eval(self._h, function, x.numel(), _ptr(x), _ptr(y)), "cf_debug_eval")
        return y

    def sync(self):
        self._check(self.lib.cf_sync(self._h), "cf_sync")

    # -- field helpers ------------------------------------------------------------------------
    def zeros(self, dtype=torch.float64):
        return torch.zeros(self.shape, dtype=dtype, device=self.device)

    def to_device(self, a):
        return torch.as_tensor(np.ascontiguousarray(a)).to(self.device)

    def field_set(self, names, optional=()):
        d = {n: self.zeros() for n in names}
        for n in optional:
            d[n] = self.zeros()
        return d

    # -- struct builders ----------------------------------------------------------------------
    @staticmethod
    def _struct(cls, fields, names):
        s = cls()
        for n in names:
            t = fields.get(n) if fields is not None else None
            if t is not None:
                assert t.is_cuda and t.is_contiguous(), n
                setattr(s, n, t.data_ptr())
        return s

    def source_struct(self, src, level1, level2, time_fraction):
        if isinstance(src, abi.AtmosSource):  # built by SnapshotWindow.source(): levels and fraction are in it
            return src
        s = abi.AtmosSource()
        shape = None
        for k, name in enumerate(abi.JRA55_VARIABLES):
            t = src[name]
            assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), name
            s.data[k] = t.data_ptr()
            shape = t.shape
        s.n_levels, s.ns_y, s.ns_x = shape
        s.level1, s.level2, s.time_fraction = level1, level2, float(time_fraction)
        return s

    def weights_struct(self, w):
        s = abi.InterpWeights()
        if w is None:
            return s
        s.separable = 1 if w.get("separable", True) else 0
        for n in ("fi", "fj", "cos_rot", "sin_rot", "latitude"):
            t = w.get(n)
            if t is not None:
                assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous(), n
                setattr(s, n, t.data_ptr())
        return s

    def ocean_struct(self, ocean):
        return self._struct(abi.OceanSurface, ocean, ("T", "S", "u", "v", "mask"))

    def exchange_struct(self, atmos):
        return self._struct(abi.ExchangeFields, atmos, EXCHANGE_NAMES)

    def fluxes_struct(self, fluxes):
        return self._struct(abi.InterfaceFluxes, fluxes, FLUX_NAMES + FLUX_OPTIONAL + ("iterations",))

    def ice_struct(self, ice):
        return None if ice is None else self._struct(abi.SeaIceFields, ice, ICE_NAMES)

    def net_struct(self, net):
        return self._struct(abi.NetOceanFluxes, net, NET_NAMES)

    # -- the hot path ---------------------------------------------------------------------------
    def interpolate_atmosphere_state(self, src, weights, atmos, level1=0, level2=1, time_fraction=0.0):
        s = self.source_struct(src, level1, level2, time_fraction)
        w = self.weights_struct(weights)
        e = self.exchange_struct(atmos)
        self._check(self.lib.cf_interpolate_atmosphere_state(self._h, C.byref(s), C.byref(w), C.byref(e)),
                    "cf_interpolate_atmosphere_state")

    def compute_atmosphere_ocean_fluxes(self, ocean, atmos, fluxes):
        o, e, f = self.ocean_struct(ocean), self.exchange_struct(atmos), self.fluxes_struct(fluxes)
        self._check(self.lib.cf_compute_atmosphere_ocean_fluxes(self._h, C.byref(o), C.byref(e), C.byref(f)),
                    "cf_compute_atmosphere_ocean_fluxes")

    def set_sea_ice_formulation(self, ice_flux_params, sea_ice_params=None):
        """atmosphere_sea_ice_fluxes + SkinTemperature(ConductiveFlux) properties of the
        atmosphere–sea-ice interface (ComponentInterfaces, omip_simulation.jl:139-158)."""
        if sea_ice_params is None:
            sea_ice_params = abi.SeaIceParams()
            self._check(self.lib.cf_default_sea_ice_params(C.byref(sea_ice_params)), "cf_default_sea_ice_params")
        self._check(self.lib.cf_set_sea_ice_formulation(self._h, C.byref(ice_flux_params), C.byref(sea_ice_params)),
                    "cf_set_sea_ice_formulation")

    def compute_atmosphere_sea_ice_fluxes(self, ice_state, ocean, atmos, fluxes):
        st = self._struct(abi.SeaIceState, ice_state,
                          ("concentration", "thickness", "top_temperature", "u", "v", "albedo", "snow_thickness"))
        o, e, f = self.ocean_struct(ocean), self.exchange_struct(atmos), self.fluxes_struct(fluxes)
        self._check(self.lib.cf_compute_atmosphere_sea_ice_fluxes(self._h, C.byref(st), C.byref(o), C.byref(e),
                                                                  C.byref(f)),
                    "cf_compute_atmosphere_sea_ice_fluxes")

    def compute_net_sea_ice_fluxes(self, ice_state, ocean, atmos, ai_fluxes, out, frazil_heat=None, interface_heat=None):
        """compute_net_sea_ice_fluxes!: out = dict(top_heat=…, bottom_heat=…)."""
        st = self._struct(abi.SeaIceState, ice_state, ("concentration", "thickness", "top_temperature", "albedo", "snow_thickness"))
        o, e, f = self.ocean_struct(ocean), self.exchange_struct(atmos), self.fluxes_struct(ai_fluxes)
        n = self._struct(abi.NetSeaIceFluxes, out, ("top_heat", "bottom_heat"))
        self._check(self.lib.cf_compute_net_sea_ice_fluxes(
            self._h, C.byref(st), C.byref(o), C.byref(e), C.byref(f),
            frazil_heat.data_ptr() if frazil_heat is not None else None,
            interface_heat.data_ptr() if interface_heat is not None else None, C.byref(n)),
            "cf_compute_net_sea_ice_fluxes")

    def default_sea_ice_albedo_params(self):
        p = abi.SeaIceAlbedoParams()
        self._check(self.lib.cf_default_sea_ice_albedo_params(C.byref(p)), "cf_default_sea_ice_albedo_params")
        return p

    def set_sea_ice_albedo(self, params=None):
        """SeaIceAlbedo(hi, hs, Ts) (CCSM3, atmosphere.jl:30-44) wherever the sea-ice state carries no albedo field."""
        self._check(self.lib.cf_set_sea_ice_albedo(self._h, C.byref(params) if params is not None else None),
                    "cf_set_sea_ice_albedo")

    def compute_sea_ice_albedo(self, params, thickness, snow_thickness, top_temperature, out):
        self._check(self.lib.cf_compute_sea_ice_albedo(self._h, C.byref(params), _ptr(thickness), _ptr(snow_thickness),
                                                       _ptr(top_temperature), _ptr(out)), "cf_compute_sea_ice_albedo")

    def default_ice_ocean_params(self, **kw):
        p = abi.IceOceanParams()
        self._check(self.lib.cf_default_ice_ocean_params(C.byref(p)), "cf_default_ice_ocean_params")
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def compute_sea_ice_ocean_fluxes(self, params, ocean, concentration, x_stress, y_stress, out):
        """compute_sea_ice_ocean_fluxes!: ThreeEquationHeatFlux(MomentumBasedFrictionVelocity) + frazil
        (omip_simulation.jl:71-77).  out: dict interface_heat, salt_flux[, frazil_heat, friction_velocity]."""
        o = self.ocean_struct(ocean)
        f = self._struct(abi.IceOceanFluxes, out, ("interface_heat", "salt_flux", "frazil_heat", "friction_velocity"))
        self._check(self.lib.cf_compute_sea_ice_ocean_fluxes(self._h, C.byref(params), C.byref(o), _ptr(concentration),
                                                             _ptr(x_stress), _ptr(y_stress), C.byref(f)),
                    "cf_compute_sea_ice_ocean_fluxes")

    def interpolate_land_freshwater(self, friver, licalvf, weights, out, level1=0, level2=1, time_fraction=0.0):
        """JRA55PrescribedLand (atmosphere.jl:46): friver + licalvf windows [n, ns_y, ns_x] float32 → one ocean-grid field."""
        s = abi.LandSource()
        assert friver.dtype == torch.float32 and friver.is_cuda and friver.is_contiguous()
        s.friver = friver.data_ptr()
        s.licalvf = licalvf.data_ptr() if licalvf is not None else None
        s.n_levels, s.ns_y, s.ns_x = friver.shape
        s.level1, s.level2, s.time_fraction = level1, level2, float(time_fraction)
        w = self.weights_struct(weights)
        self._check(self.lib.cf_interpolate_land_freshwater(self._h, C.byref(s), C.byref(w), _ptr(out)),
                    "cf_interpolate_land_freshwater")

    def set_land_freshwater(self, field):
        self._land = field      # keep the tensor alive: the library borrows the pointer
        self._check(self.lib.cf_set_land_freshwater(self._h, _ptr(field)), "cf_set_land_freshwater")

    def materialize_salinity_restoring(self, piston_velocity, target, ocean, out):
        """SurfaceFluxRestoring as the additional flux of MultipleFluxes (omip_simulation.jl:175-206, 507-523)."""
        o = self.ocean_struct(ocean)
        self._check(self.lib.cf_materialize_salinity_restoring(self._h, float(piston_velocity), _ptr(target), C.byref(o), _ptr(out)),
                    "cf_materialize_salinity_restoring")

    def compute_net_ocean_fluxes(self, ocean, atmos, fluxes, net, ice=None, weights=None):
        o, e, f = self.ocean_struct(ocean), self.exchange_struct(atmos), self.fluxes_struct(fluxes)
        i = self.ice_struct(ice)
        w = self.weights_struct(weights)
        n = self.net_struct(net)
        self._check(self.lib.cf_compute_net_ocean_fluxes(self._h, C.byref(o), C.byref(e), C.byref(f),
                                                         C.byref(i) if i is not None else None,
                                                         C.byref(w), C.byref(n)),
                    "cf_compute_net_ocean_fluxes")

    def update_state(self, src, weights, ocean, atmos, fluxes, net, ice=None, level1=0, level2=1,
                     time_fraction=0.0):
        s = self.source_struct(src, level1, level2, time_fraction)
        w = self.weights_struct(weights)
        o, e, f = self.ocean_struct(ocean), self.exchange_struct(atmos), self.fluxes_struct(fluxes)
        i = self.ice_struct(ice)
        n = self.net_struct(net)
        self._check(self.lib.cf_update_state(self._h, C.byref(s), C.byref(w), C.byref(o), C.byref(e),
                                             C.byref(f), C.byref(i) if i is not None else None, C.byref(n)),
                    "cf_update_state")

    def update_state_sea_ice(self, src, weights, ocean, atmos, fluxes, net, ice, ice_state, ai_fluxes, net_ice,
                             frazil_heat=None, interface_heat=None, level1=0, level2=1, time_fraction=0.0):
        """update_state! of a model with sea ice: the ocean path, then the atmosphere–sea-ice interface and the
        net sea-ice fluxes (cf_update_state_sea_ice)."""
        s = self.source_struct(src, level1, level2, time_fraction)
        w = self.weights_struct(weights)
        o, e, f = self.ocean_struct(ocean), self.exchange_struct(atmos), self.fluxes_struct(fluxes)
        i = self.ice_struct(ice)
        n = self.net_struct(net)
        st = self._struct(abi.SeaIceState, ice_state, ("concentration", "thickness", "top_temperature", "u", "v", "albedo", "snow_thickness"))
        af = self.fluxes_struct(ai_fluxes)
        ni = self._struct(abi.NetSeaIceFluxes, net_ice, ("top_heat", "bottom_heat"))
        self._check(self.lib.cf_update_state_sea_ice(
            self._h, C.byref(s), C.byref(w), C.byref(o), C.byref(e), C.byref(f), C.byref(i) if i is not None else None,
            C.byref(n), C.byref(st), C.byref(af), frazil_heat.data_ptr() if frazil_heat is not None else None,
            interface_heat.data_ptr() if interface_heat is not None else None, C.byref(ni)), "cf_update_state_sea_ice")

    def time_stage(self, stage, launches, *, src=None, weights=None, ocean=None, atmos=None, fluxes=None,
                   net=None, ice=None, level1=0, level2=1, time_fraction=0.0):
        """Average ms per launch of one stage, measured with HIP events on the launch stream."""
        s = self.source_struct(src, level1, level2, time_fraction) if src is not None else abi.AtmosSource()
        w = self.weights_struct(weights)
        o, e, f = self.ocean_struct(ocean), self.exchange_struct(atmos), self.fluxes_struct(fluxes)
        i = self.ice_struct(ice)
        n = self.net_struct(net)
        ms = C.c_double()
        self._check(self.lib.cf_time_stage(self._h, stage, launches, C.byref(s), C.byref(w), C.byref(o),
                                           C.byref(e), C.byref(f), C.byref(i) if i is not None else None,
                                           C.byref(n), C.byref(ms)), "cf_time_stage")
        return ms.value

    def ensure_chunk_table(self, mask):
        """Build the solver's schedule for `mask` now instead of inside the first step."""
        self._check(self.lib.cf_ensure_chunk_table(self._h, _ptr(mask)), "cf_ensure_chunk_table")

    def debug_chunk_table(self):
        """(begins, wet_counts, lists_valid) of the chunk table as the device built it (cf_debug_chunk_table, after
        ensure_chunk_table or a solve): int32 arrays of n + 1 and n entries and whether the static wet lists are in use."""
        n, valid = C.c_int(), C.c_int()
        capacity = 1024
        while True:
            begins, counts = np.zeros(capacity, dtype=np.int32), np.zeros(capacity, dtype=np.int32)
            rc = self.lib.cf_debug_chunk_table(self._h, begins.ctypes.data_as(C.POINTER(C.c_int)),
                                               counts.ctypes.data_as(C.POINTER(C.c_int)), capacity, C.byref(n), C.byref(valid))
            if rc != 0 and n.value + 1 > capacity:   # too few ints: *n_chunks says how many
                capacity = n.value + 1
                continue
            self._check(rc, "cf_debug_chunk_table")
            return begins[:n.value + 1].copy(), counts[:n.value].copy(), bool(valid.value)

    def debug_interp_grid(self):
        """(rows, blocks) of the tiled interpolation on this context's grid under its options (cf_debug_interp_grid): rows of 64
        cells per wave tile — automatic, or what abi.OPT_INTERP_TILE_ROWS forces — and workgroups; launches nothing."""
        rows, blocks = C.c_int(), C.c_int()
        self._check(self.lib.cf_debug_interp_grid(self._h, C.byref(rows), C.byref(blocks)), "cf_debug_interp_grid")
        return rows.value, blocks.value

    def debug_land_zero_launches(self):
        """How many ocean-solver launches of the last time_steps call wrote the land zeros (cf_debug_land_zero_launches;
        abi.OPT_LAND_ZEROS): 1 under the automatic mode, the step count under LAND_ZEROS_EVERY_LAUNCH."""
        n = C.c_int()
        self._check(self.lib.cf_debug_land_zero_launches(self._h, C.byref(n)), "cf_debug_land_zero_launches")
        return n.value

    def solver_path(self):
        """(lean_kernel, fused): which kernels cf_update_state launches for the current formulation and options; fused = 0
        three launches, 1 net fluxes in the solver's epilogue, 2 the interpolation in its prologue as well."""
        lean, fused = C.c_int(), C.c_int()
        self._check(self.lib.cf_solver_path(self._h, C.byref(lean), C.byref(fused)), "cf_solver_path")
        return bool(lean.value), fused.value

    def solver_iteration_path(self):
        """abi.SOLVER_PATH_EXACT or abi.SOLVER_PATH_CERTIFIED: what the ocean solve would run with the current options."""
        path = C.c_int()
        self._check(self.lib.cf_solver_iteration_path(self._h, C.byref(path)), "cf_solver_iteration_path")
        return path.value

    def solver_latency_layout(self):
        """True when the exact path's launch would take the kernels laid out for one or two waves per SIMD
        (CF_OPT_LATENCY_LAYOUT; valid once the chunk table is built)."""
        layout = C.c_int()
        self._check(self.lib.cf_solver_latency_layout(self._h, C.byref(layout)), "cf_solver_latency_layout")
        return bool(layout.value)

    def time_copy(self, nbytes, launches=20):
        a = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)
        b = torch.empty_like(a)
        ms = C.c_double()
        self._check(self.lib.cf_time_copy(self._h, _ptr(b), _ptr(a), nbytes, launches, C.byref(ms)),
                    "cf_time_copy")
        return ms.value

    def normalize_salinity_flux(self, flux, mask, additional=None, area=None, mean_out=None):
        """NormalizeSalinity (omip_simulation.jl:182-220): flux -= area-weighted mean over wet cells."""
        self._check(self.lib.cf_normalize_salinity_flux(self._h, _ptr(flux), _ptr(additional), _ptr(area), _ptr(mask),
                                                        _ptr(mean_out)), "cf_normalize_salinity_flux")

    def normalize_salinity_flux_exact(self, flux, mask, additional=None, area=None, mean_out=None):
        """NormalizeSalinity with exact sums (cf_normalize_salinity_flux_exact): the mean's bits do not depend on how the globe is
        cut into slabs; summed over the reduction world when one is connected on more than one rank (peer_reduce_connect)."""
        self._check(self.lib.cf_normalize_salinity_flux_exact(self._h, _ptr(flux), _ptr(additional), _ptr(area), _ptr(mask),
                                                              _ptr(mean_out)), "cf_normalize_salinity_flux_exact")

    def debug_salinity_sums_exact(self, flux, mask, additional=None, area=None):
        """This rank's exact sums (fl(Σ fl(fl(flux + additional) · area)), fl(Σ area)) over the wet interior and the counts of
        NaN, +Inf and −Inf terms of the first (cf_debug_salinity_sums_exact).  Synchronises; writes nothing to `flux`."""
        sums, counts = (C.c_double * 2)(), (C.c_ulonglong * 3)()
        self._check(self.lib.cf_debug_salinity_sums_exact(self._h, _ptr(flux), _ptr(additional), _ptr(area), _ptr(mask), sums, counts),
                    "cf_debug_salinity_sums_exact")
        return (sums[0], sums[1]), tuple(int(c) for c in counts)

    def profile_enable(self, max_records):
        self._check(self.lib.cf_profile_enable(self._h, max_records), "cf_profile_enable")

    def profile_read(self, kernel):
        """(average ms, records) of kernel 0 (interpolate), 1 (atmosphere–ocean fluxes) or 2 (net fluxes)."""
        ms, n = C.c_double(), C.c_int()
        self._check(self.lib.cf_profile_read(self._h, kernel, C.byref(ms), C.byref(n)), "cf_profile_read")
        return ms.value, n.value

    def prefetch_atmosphere_state(self, src, weights, atmos_next, level1=0, level2=1, time_fraction=0.0):
        """Start the NEXT step's interpolate_atmosphere_state! on the auxiliary stream (cf_prefetch_atmosphere_state)."""
        s = self.source_struct(src, level1, level2, time_fraction)
        w = self.weights_struct(weights)
        e = self.exchange_struct(atmos_next)
        self._check(self.lib.cf_prefetch_atmosphere_state(self._h, C.byref(s), C.byref(w), C.byref(e)),
                    "cf_prefetch_atmosphere_state")

    def discard_prefetched_atmosphere_state(self):
        """Forget requested-ahead atmosphere states (cf_discard_prefetched_atmosphere_state): on leaving a stepping loop."""
        self._check(self.lib.cf_discard_prefetched_atmosphere_state(self._h), "cf_discard_prefetched_atmosphere_state")

    def prefetch_stats(self):
        """Which way every requested-ahead atmosphere state went since the context was made (cf_debug_prefetch_stats), as a
        dict of ints: requests, launched_aux / _tail / _merged / _ice_tail / _own, consumed, mismatched, voided, superseded,
        discarded, step_interpolations and pending.  requests = the five endings + pending, always."""
        st = abi.PrefetchStats()
        st.struct_size = C.sizeof(abi.PrefetchStats)
        self._check(self.lib.cf_debug_prefetch_stats(self._h, C.byref(st)), "cf_debug_prefetch_stats")
        return {n: int(getattr(st, n)) for n, _ in abi.PrefetchStats._fields_ if n != "struct_size"}

    def make_schedule(self, ocean_states, atmos_sets, *, first_level=0, time_fraction=0.0, time_fraction_increment=0.0,
                      pipeline=False, halo_backend=abi.HALO_NONE, halo_rows=0, fold_north=False):
        """cf_run_schedule for cf_time_steps; keeps the ctypes arrays alive on the returned object."""
        sch = abi.RunSchedule()
        oc = (abi.OceanSurface * len(ocean_states))(*[self.ocean_struct(o) for o in ocean_states])
        at = (abi.ExchangeFields * len(atmos_sets))(*[self.exchange_struct(a) for a in atmos_sets])
        sch.struct_size = C.sizeof(abi.RunSchedule)
        sch.n_ocean_states, sch.ocean_states = len(ocean_states), oc
        sch.n_atmos_sets, sch.atmos, sch.pipeline = len(atmos_sets), at, int(pipeline)   # False / True (within the call) / abi.PIPELINE_CONTINUING
        sch.first_level, sch.halo_backend, sch.halo_rows = first_level, halo_backend, halo_rows
        sch.fold_north = 1 if fold_north else 0
        sch.time_fraction, sch.time_fraction_increment = float(time_fraction), float(time_fraction_increment)
        sch._keep = (oc, at, ocean_states, atmos_sets)
        return sch

    def time_steps(self, first_step, nsteps, schedule, src, weights, fluxes, net, ice=None):
        """run!(simulation) of a prescribed-ocean model: nsteps × (halo rows → update_state!) inside libcoflux."""
        s = self.source_struct(src, 0, 0, 0.0)
        w = self.weights_struct(weights)
        f, n, i = self.fluxes_struct(fluxes), self.net_struct(net), self.ice_struct(ice)
        self._check(self.lib.cf_time_steps(self._h, first_step, nsteps, C.byref(schedule), C.byref(s), C.byref(w),
                                           C.byref(f), C.byref(i) if i is not None else None, C.byref(n)),
                    "cf_time_steps")

    # -- the coupled step: sea ice, land, restoring ------------------------------------------------
    ICE_STATE_NAMES = ("concentration", "thickness", "top_temperature", "u", "v", "albedo", "snow_thickness")

    def _land_struct(self, friver, licalvf, level1=0, level2=0, time_fraction=0.0):
        s = abi.LandSource()
        if friver is not None:
            assert friver.dtype == torch.float32 and friver.is_cuda and friver.is_contiguous()
            s.friver = friver.data_ptr()
            s.licalvf = licalvf.data_ptr() if licalvf is not None else None
            s.n_levels, s.ns_y, s.ns_x = friver.shape
        s.level1, s.level2, s.time_fraction = level1, level2, float(time_fraction)
        return s

    def prepare_coupled_step(self, ocean, *, weights=None, friver=None, licalvf=None, land_out=None, level1=0, level2=1,
                             time_fraction=0.0, ice_ocean_params=None, concentration=None, x_stress=None, y_stress=None,
                             ice_ocean_out=None, piston_velocity=0.0, target=None, restoring_out=None):
        """cf_prepare_coupled_step: interpolate_land_freshwater (→ land_out), compute_sea_ice_ocean_fluxes (→ the dict
        ice_ocean_out) and materialize_salinity_restoring (→ restoring_out) as one launch, same bits; a job whose output is
        None is left out."""
        p = abi.CoupledPrepare()
        p.struct_size = C.sizeof(abi.CoupledPrepare)
        p.ocean = self.ocean_struct(ocean)
        if land_out is not None:
            p.weights = self.weights_struct(weights)
            p.land = self._land_struct(friver, licalvf, level1, level2, time_fraction)
            p.land_freshwater = land_out.data_ptr()
        if ice_ocean_out is not None:
            p.ice_ocean = ice_ocean_params
            p.concentration, p.x_stress, p.y_stress = _ptr(concentration), _ptr(x_stress), _ptr(y_stress)
            p.ice_ocean_fluxes = self._struct(abi.IceOceanFluxes, ice_ocean_out,
                                              ("interface_heat", "salt_flux", "frazil_heat", "friction_velocity"))
        if restoring_out is not None:
            p.piston_velocity, p.target_salinity, p.restoring_buffer = float(piston_velocity), _ptr(target), restoring_out.data_ptr()
        self._check(self.lib.cf_prepare_coupled_step(self._h, C.byref(p)), "cf_prepare_coupled_step")

    def make_coupled_step(self, ice_states, skin_temperature, ai_fluxes, net_ice, *, friver=None, licalvf=None, land_out=None,
                          land_first_level=0, land_time_fraction=0.0, land_time_fraction_increment=0.0, ice_ocean_params=None,
                          ice_ocean_fluxes=None, piston_velocity=0.0, target=None, restoring_out=None, normalize=False, area=None,
                          mean_out=None):
        """cf_coupled_step for time_steps_coupled; keeps the ctypes array and the tensors alive on the returned object.
        `ice_states`: dicts of ICE_STATE_NAMES (top_temperature is ignored: `skin_temperature` is carried); `ice_ocean_fluxes`:
        dict interface_heat, salt_flux[, frazil_heat, friction_velocity] — computed each step when `ice_ocean_params` is
        given, taken as given otherwise."""
        k = abi.CoupledStep()
        k.struct_size = C.sizeof(abi.CoupledStep)
        st = (abi.SeaIceState * max(len(ice_states), 1))(*[self._struct(abi.SeaIceState, s, self.ICE_STATE_NAMES) for s in ice_states])
        k.n_ice_states, k.ice_states = len(ice_states), st
        k.skin_temperature = _ptr(skin_temperature)
        k.ai_fluxes = self.fluxes_struct({n: t for n, t in (ai_fluxes or {}).items() if n != "temperature"})
        k.net_ice = self._struct(abi.NetSeaIceFluxes, net_ice, ("top_heat", "bottom_heat"))
        k.land = self._land_struct(friver, licalvf)
        k.land_first_level, k.land_time_fraction = int(land_first_level), float(land_time_fraction)
        k.land_time_fraction_increment = float(land_time_fraction_increment)
        k.land_freshwater = _ptr(land_out)
        if ice_ocean_params is not None:
            k.compute_ice_ocean, k.ice_ocean = 1, ice_ocean_params
        k.ice_ocean_fluxes = self._struct(abi.IceOceanFluxes, ice_ocean_fluxes, ("interface_heat", "salt_flux", "frazil_heat", "friction_velocity"))
        k.piston_velocity, k.target_salinity, k.restoring_buffer = float(piston_velocity), _ptr(target), _ptr(restoring_out)
        # normalize: False / True (cf_normalize_salinity_flux) / "exact" (cf_normalize_salinity_flux_exact: abi.NORMALIZE_EXACT)
        if isinstance(normalize, str) and normalize != "exact":
            raise ValueError(f'normalize = {normalize!r}: False, True or "exact"')
        k.normalize_salinity = abi.NORMALIZE_EXACT if isinstance(normalize, str) and normalize == "exact" else int(bool(normalize))
        k.area, k.mean_out = _ptr(area), _ptr(mean_out)
        k._keep = (st, ice_states, skin_temperature, ai_fluxes, net_ice, friver, licalvf, land_out, ice_ocean_fluxes, target, restoring_out,
                   area, mean_out)
        return k

    def time_steps_coupled(self, first_step, nsteps, schedule, src, weights, fluxes, net, ice, coupled):
        """run!(simulation) of the OMIP configuration inside libcoflux (cf_time_steps_coupled): per step the fold, the
        preamble (land, ice–ocean exchange, restoring), update_state_sea_ice with the carried skin temperature, and
        NormalizeSalinity.  `ice`: the partition's stresses (dict x_stress, y_stress) or None."""
        s = self.source_struct(src, 0, 0, 0.0)
        w = self.weights_struct(weights)
        f, n, i = self.fluxes_struct(fluxes), self.net_struct(net), self.ice_struct(ice)
        self._check(self.lib.cf_time_steps_coupled(self._h, first_step, nsteps, C.byref(schedule), C.byref(s), C.byref(w), C.byref(f),
                                                   C.byref(i) if i is not None else None, C.byref(n),
                                                   C.byref(coupled) if coupled is not None else None), "cf_time_steps_coupled")

    # -- time averages ----------------------------------------------------------------------------
    def average(self, sources, means):
        """A device-side running mean of `sources` into `means` (cf_average_create): lists of up to abi.AVERAGE_MAX_FIELDS
        ocean-grid float64 fields; collect(weight) after each sample, read the means, reset() for the next window."""
        return TimeAverager(self, sources, means)

    def derived_average(self, terms, cos_rotation=None, sin_rotation=None, max_workgroups=0):
        """A device-side running mean of derived quantities (cf_average_create_derived), a TimeAverager like average()'s.
        `terms`: up to abi.AVERAGE_MAX_FIELDS tuples (kind, a, b, scale, flags, mean) — kind a name of TERM_KINDS or
        abi.TERM_*, `a` / `b` / `mean` ocean-grid float64 fields (b None where the kind has none), the sample is x · scale;
        `cos_rotation` / `sin_rotation`: ocean-grid float64 fields, for "east" / "north" terms.  Where a kind reads [i+1] /
        [j+1] the caller has filled the first east halo column / north halo row of that field.  `max_workgroups` caps the
        launch (0: the library's; scheduling only)."""
        return TimeAverager.derived(self, terms, cos_rotation, sin_rotation, max_workgroups)

    def budget_average(self, terms, *, ocean=None, atmos=None, fluxes=None, ice=None, frazil_heat=None, land_freshwater=None,
                       weights=None, max_workgroups=0):
        """A device-side running mean of parts of the net heat and salt flux (cf_average_create_budget), a TimeAverager like
        average()'s.  `terms`: up to abi.AVERAGE_MAX_FIELDS tuples (kind, scale, mean) — kind a name of BUDGET_KINDS or
        abi.BUDGET_*, the sample is x · scale, `mean` an ocean-grid float64 field.  The inputs are those the net fluxes were
        computed from: the dicts `ocean` (S, mask), `atmos` (Qs, Ql, Mp), `fluxes` (sensible_heat, latent_heat, water_vapor,
        temperature), `ice` (concentration, interface_heat, salt_flux), the fields `frazil_heat` and `land_freshwater`, and
        `weights` (latitude, separable: the latitude-dependent albedo only).  Whatever no requested kind reads may be left
        out.  The parameters are the context's at each collection."""
        return TimeAverager.budget(self, terms, ocean, atmos, fluxes, ice, frazil_heat, land_freshwater, weights, max_workgroups)

    def attach_average(self, averager, stride=1, step_weight=1.0, slot=0):
        """time_steps() and time_steps_coupled() collect `averager` after every step s with (s + 1) % stride == 0, weight
        stride · step_weight; None empties the slot.  `slot`: 0 … abi.ATTACHED_AVERAGES_MAX − 1, collected in slot order, each
        with its own stride and weight (cf_attach_average_slot; slot 0 is cf_attach_average's)."""
        h = averager._h if averager is not None else None
        slot = int(slot)
        if slot == 0:
            rc, what = self.lib.cf_attach_average(self._h, h, int(stride), float(step_weight)), "cf_attach_average"
        else:
            rc, what = self.lib.cf_attach_average_slot(self._h, slot, h, int(stride), float(step_weight)), "cf_attach_average_slot"
        self._check(rc, what)
        if not hasattr(self, "_attached_averages"):
            self._attached_averages = {}
        self._attached_averages[slot] = averager   # kept alive while attached

    # -- surface integrals ------------------------------------------------------------------------
    def integrals(self, entries, area=None, mask=None, region=None, capacity=1024, max_workgroups=0):
        """A device-side time series of area-weighted, masked, regional integrals (cf_integrals_create).  `entries`: up to
        abi.INTEGRALS_MAX_ENTRIES tuples (kind, a, b, threshold, region_bit) — kind "one" | "field" | "product" | "above" or
        abi.INTEGRAND_*, `a` / `b` ocean-grid float64 fields (None where the kind has none); trailing items may be left out.
        `area`: float64 cell areas, `mask`: the context's wet mask, `region`: uint8 region bits (all ocean-grid arrays)."""
        return SurfaceIntegrator(self, entries, area, mask, region, capacity, max_workgroups)

    def _attach_series(self, family, handle, stride, time_origin, step_seconds):
        setattr(self, "_attached_" + family, handle)   # kept alive while attached
        h = handle._h if handle is not None else None
        self._check(getattr(self.lib, "cf_attach_" + family)(self._h, h, int(stride), float(time_origin), float(step_seconds)),
                    "cf_attach_" + family)

    def attach_integrals(self, integrator, stride=1, time_origin=0.0, step_seconds=1.0):
        """time_steps() appends a record of `integrator` after every step s with (s + 1) % stride == 0, stamped
        time_origin + (s + 1) · step_seconds (cf_attach_integrals); None detaches."""
        self._attach_series("integrals", integrator, stride, time_origin, step_seconds)

    # -- surface monitor --------------------------------------------------------------------------
    def monitor(self, entries, mask=None, first_cell=0, capacity=1024, max_workgroups=0, row_length=0):
        """A device-side time series of extrema, non-finite counts and state hashes (cf_monitor_create).  `entries`: up to
        abi.MONITOR_MAX_ENTRIES ocean-grid float64 fields or (field, "value" | "abs") pairs (abi.MONITOR_* work too);
        `mask`: the context's wet mask; `first_cell`: the global index j0·Nx + i0 of this slab's or tile's interior cell
        (0, 0); `row_length`: the global row length Nx of a tile's surface (0: the context's nx)."""
        return SurfaceMonitor(self, entries, mask, first_cell, capacity, max_workgroups, row_length)

    def attach_monitor(self, monitor, stride=1, time_origin=0.0, step_seconds=1.0):
        """time_steps() appends a record of `monitor` after every step s with (s + 1) % stride == 0, stamped
        time_origin + (s + 1) · step_seconds (cf_attach_monitor), after the attached averager and integrator; None detaches."""
        self._attach_series("monitor", monitor, stride, time_origin, step_seconds)

    # -- calendar-binned means --------------------------------------------------------------------
    def climatology(self, sources, totals, bins, n_bins, max_workgroups=0):
        """Device-side calendar-binned running means (cf_climatology_create): per field of `sources` (up to
        abi.CLIMATOLOGY_MAX_FIELDS ocean-grid float64 fields) a total mean `totals[k]` (an ocean-grid field, or None: that
        field keeps no total) and a block `bins[k]` of shape (n_bins,) + ctx.shape; collect(bin, weight) after each sample."""
        return Climatology(self, sources, totals, bins, n_bins, max_workgroups)

    def attach_climatology(self, clim, table=None, stride=1, step_weight=1.0, time_origin=0.0, step_seconds=1.0):
        """time_steps() and time_steps_coupled() collect `clim` after every step s with (s + 1) % stride == 0, after the
        attached averagers and before the integrator and the monitor: the step is stamped time_origin + (s + 1) · step_seconds,
        `table` = (edges, bin_of_interval) — as coflux.models.calendar_bins builds it; the library copies it — gives the bin
        (−1: not collected), the weight is stride · step_weight (cf_attach_climatology).  None detaches."""
        if clim is None:
            self._check(self.lib.cf_attach_climatology(self._h, None, 1, 1.0, 0.0, 0.0, None, None, 0), "cf_attach_climatology")
            self._attached_climatology = None
            return
        edges = np.ascontiguousarray(table[0], dtype=np.float64)
        bin_of_interval = np.ascontiguousarray(table[1], dtype=np.int32)
        if edges.ndim != 1 or bin_of_interval.shape != (max(edges.size - 1, 0),):
            raise ValueError(f"attach_climatology: {edges.size} edges bound {edges.size - 1} intervals, got {bin_of_interval.shape}")
        self._check(self.lib.cf_attach_climatology(self._h, clim._h, int(stride), float(step_weight), float(time_origin), float(step_seconds),
                                                   edges.ctypes.data_as(abi.c_double_p), bin_of_interval.ctypes.data_as(abi.c_int32_p),
                                                   int(edges.size)), "cf_attach_climatology")
        self._attached_climatology = clim   # kept alive while attached

    # -- staged datasets ---------------------------------------------------------------------------
    def dataset(self, ns_x, ns_y, times, weights, period=0.0, periodic_x=True, max_sweeps=-1, fill_value=0.0, sweeps_per_launch=0,
                max_workgroups=0):
        """A dataset staged on the device (cf_dataset_create): len(times) levels of an ns_y × ns_x source grid, each
        stage(level, plane) land-inpainted, interpolated through `weights` (as interpolate_land_freshwater takes them) onto an
        ocean-grid array the handle owns; evaluate(time) blends two levels — cyclically when period > 0, clamped otherwise."""
        return Dataset(self, ns_x, ns_y, times, weights, period, periodic_x, max_sweeps, fill_value, sweeps_per_launch, max_workgroups)

    def materialize_dataset_restoring(self, piston_velocity, dataset, time, ocean, out):
        """materialize_salinity_restoring with S★ formed per cell from `dataset` at `time` (cf_materialize_dataset_restoring)."""
        o = self.ocean_struct(ocean)
        self._check(self.lib.cf_materialize_dataset_restoring(self._h, float(piston_velocity), dataset._h, float(time), C.byref(o), _ptr(out)),
                    "cf_materialize_dataset_restoring")

    def attach_restoring_dataset(self, dataset, time_origin=0.0, step_seconds=1.0):
        """Step s of time_steps_coupled() restores toward `dataset` at time_origin + s · step_seconds, inside the preamble's
        launch; the block's target_salinity is then None (cf_attach_restoring_dataset).  None detaches."""
        h = dataset._h if dataset is not None else None
        self._check(self.lib.cf_attach_restoring_dataset(self._h, h, float(time_origin), float(step_seconds)), "cf_attach_restoring_dataset")
        self._attached_restoring_dataset = dataset   # kept alive while attached

    # -- checkpoint and pickup --------------------------------------------------------------------
    def checkpoint(self, direct=False, max_workgroups=0):
        """A checkpoint handle (cf_checkpoint_create): register arrays and handles, capture() … wait() → image,
        restore(image) in the next process.  `direct`: no device staging image."""
        return Checkpoint(self, direct, max_workgroups)

    # -- sparse surface operators -----------------------------------------------------------------
    def regridder(self, row_ptr, col, weight, mask=None, mode="mean", max_workgroups=0):
        """A fixed sparse surface operator on the device (cf_regrid_create): CSR over destination rows — row_ptr (n_rows + 1),
        col (interior cell numbers j·nx + i) and weight (≥ 0), host arrays as coflux.regridding builds them; `mask`: the
        context's wet mask (ocean-grid device array); mode "mean" (Σ w x / Σ w over the wet entries, NaN where that is 0) or
        "sum".  apply(sources) regrids up to abi.REGRID_MAX_FIELDS ocean-grid fields in one pass."""
        return SurfaceRegridder(self, row_ptr, col, weight, mask, mode, max_workgroups)

    # -- peer-direct halo rows / tripolar fold -----------------------------------------------------
    def peer_halo_export(self, max_fields=4, max_rows=2):
        buf = C.create_string_buffer(abi.PEER_HANDLE_BYTES)
        self._check(self.lib.cf_peer_halo_export(self._h, max_fields, max_rows, buf), "cf_peer_halo_export")
        return buf.raw

    def peer_halo_connect(self, south, north, rank, nranks):
        sb = C.create_string_buffer(south, abi.PEER_HANDLE_BYTES) if south is not None else None
        nb = C.create_string_buffer(north, abi.PEER_HANDLE_BYTES) if north is not None else None
        self._check(self.lib.cf_peer_halo_connect(self._h, sb, nb, rank, nranks), "cf_peer_halo_connect")

    def peer_reduce_export(self):
        """This context's reduce mailbox as a HIP IPC handle (cf_peer_reduce_export)."""
        buf = C.create_string_buffer(abi.PEER_HANDLE_BYTES)
        self._check(self.lib.cf_peer_reduce_export(self._h, buf), "cf_peer_reduce_export")
        return buf.raw

    def peer_reduce_connect(self, handles, rank, nranks):
        """Join the reduction world of the exact sums (cf_peer_reduce_connect): `handles` is every rank's handle in rank order
        (None for a world of one)."""
        blob = None
        if handles is not None:
            assert len(handles) == nranks and all(len(h) == abi.PEER_HANDLE_BYTES for h in handles)
            blob = C.create_string_buffer(b"".join(handles), nranks * abi.PEER_HANDLE_BYTES)
        self._check(self.lib.cf_peer_reduce_connect(self._h, blob, rank, nranks), "cf_peer_reduce_connect")

    def peer_halo_stats(self):
        """(exchanges issued, of which as riders of a solver launch: CF_OPT_HALO_IN_SOLVER_LAUNCH)."""
        a, b = C.c_ulonglong(), C.c_ulonglong()
        self._check(self.lib.cf_peer_halo_stats(self._h, C.byref(a), C.byref(b)), "cf_peer_halo_stats")
        return a.value, b.value

    def fold_counts(self):
        """(fold launches of their own, exchange launches whose north side was the tripolar fold) since the context was created
        (cf_debug_fold_counts)."""
        a, b = C.c_longlong(), C.c_longlong()
        self._check(self.lib.cf_debug_fold_counts(self._h, C.byref(a), C.byref(b)), "cf_debug_fold_counts")
        return a.value, b.value

    def halo_exchange_rows_peer(self, tensors, rows=2):
        arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        self._check(self.lib.cf_halo_exchange_rows_peer(self._h, arr, len(tensors), rows), "cf_halo_exchange_rows_peer")

    def fold_north_halo(self, tensors, locations, signs, rows=2):
        n = len(tensors)
        arr = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
        loc = (C.c_int * n)(*locations)
        sg = (C.c_double * n)(*signs)
        self._check(self.lib.cf_fold_north_halo(self._h, arr, loc, sg, n, rows), "cf_fold_north_halo")

    # -- the tile world: a px × py partition (cf_peer_tile_*) -----------------------------------------
    def peer_tile_export(self, max_fields=4, max_rows=2, max_cols=3):
        """This context's tile mailbox as a HIP IPC handle (cf_peer_tile_export).  max_cols: ring + 1, and one more on the top
        row of a tripolar world with px > 1."""
        buf = C.create_string_buffer(abi.PEER_HANDLE_BYTES)
        self._check(self.lib.cf_peer_tile_export(self._h, max_fields, max_rows, max_cols, buf), "cf_peer_tile_export")
        return buf.raw

    def peer_tile_connect(self, handles, px, py, rank, tripolar):
        """Join the px × py tile world as rank = p + px · q (cf_peer_tile_connect): `handles` is every rank's handle in rank
        order (None for a world of one)."""
        blob = None
        if handles is not None:
            assert all(len(h) == abi.PEER_HANDLE_BYTES for h in handles)
            blob = C.create_string_buffer(b"".join(handles), len(handles) * abi.PEER_HANDLE_BYTES)
        self._check(self.lib.cf_peer_tile_connect(self._h, blob, px, py, rank, 1 if tripolar else 0), "cf_peer_tile_connect")

    def halo_exchange_tile_peer(self, tensors, locations=None, signs=None, rows=2, fold_north=False):
        """One tile exchange of `tensors` (cf_halo_exchange_tile_peer): locations (abi.FOLD_*) and signs are read where
        fold_north is set — on every rank of the top row of a tripolar world."""
        n = len(tensors)
        arr = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
        loc = (C.c_int * n)(*locations) if locations is not None else None
        sg = (C.c_double * n)(*signs) if signs is not None else None
        self._check(self.lib.cf_halo_exchange_tile_peer(self._h, arr, loc, sg, n, rows, 1 if fold_north else 0), "cf_halo_exchange_tile_peer")

    def tile_stats(self):
        """(exchanges issued, x-phase launches, exchanges that sent a fold to a partner) since the context was created
        (cf_peer_tile_stats)."""
        a, b, c = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        self._check(self.lib.cf_peer_tile_stats(self._h, C.byref(a), C.byref(b), C.byref(c)), "cf_peer_tile_stats")
        return a.value, b.value, c.value

    # -- RCCL halo rows -------------------------------------------------------------------------
    def comm_init(self, unique_id: bytes, rank, nranks):
        buf = C.create_string_buffer(unique_id, abi.COMM_ID_BYTES)
        self._check(self.lib.cf_comm_init(self._h, buf, rank, nranks), "cf_comm_init")

    def comm_count(self):
        """(nranks, rank, device) as RCCL itself reports them for the communicator of comm_init (cf_comm_count)."""
        n, r, d = C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.cf_comm_count(self._h, C.byref(n), C.byref(r), C.byref(d)), "cf_comm_count")
        return n.value, r.value, d.value

    def halo_exchange_rows(self, tensors, rows=1):
        arr = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        self._check(self.lib.cf_halo_exchange_rows(self._h, arr, len(tensors), rows), "cf_halo_exchange_rows")


TERM_KINDS = dict(field=abi.TERM_FIELD, product=abi.TERM_PRODUCT, center_x=abi.TERM_CENTER_X, center_y=abi.TERM_CENTER_Y,
                  center_x_square=abi.TERM_CENTER_X_SQUARE, center_y_square=abi.TERM_CENTER_Y_SQUARE,
                  kinetic_energy=abi.TERM_KINETIC_ENERGY, east=abi.TERM_EAST, north=abi.TERM_NORTH)


BUDGET_KINDS = dict(heat_shortwave=abi.BUDGET_HEAT_SHORTWAVE, heat_longwave_up=abi.BUDGET_HEAT_LONGWAVE_UP,
                    heat_longwave_down=abi.BUDGET_HEAT_LONGWAVE_DOWN, heat_sensible=abi.BUDGET_HEAT_SENSIBLE,
                    heat_latent=abi.BUDGET_HEAT_LATENT, heat_atmosphere_ocean=abi.BUDGET_HEAT_ATMOSPHERE_OCEAN,
                    heat_ice_ocean=abi.BUDGET_HEAT_ICE_OCEAN, heat_frazil=abi.BUDGET_HEAT_FRAZIL, heat_net=abi.BUDGET_HEAT_NET,
                    salt_evaporation=abi.BUDGET_SALT_EVAPORATION, salt_precipitation=abi.BUDGET_SALT_PRECIPITATION,
                    salt_atmosphere_ocean=abi.BUDGET_SALT_ATMOSPHERE_OCEAN, salt_ice_ocean=abi.BUDGET_SALT_ICE_OCEAN,
                    salt_land=abi.BUDGET_SALT_LAND, salt_net=abi.BUDGET_SALT_NET)


class _ChildHandle:
    """What TimeAverager, Climatology, SurfaceIntegrator, SurfaceMonitor, SurfaceRegridder, Checkpoint and SnapshotWindow share: a handle `_h` made on the context
    `ctx` that may outlive it (the library then fails every call but the `_destroy` one with "… has been destroyed")."""
    _destroy = None   # name of the cf_*_destroy entry point

    def _adopt(self, ctx):
        self.ctx, self.lib, self._h = ctx, ctx.lib, C.c_void_p()

    def _check(self, rc, what):
        if rc != 0:
            raise CofluxError(f"{what} failed ({rc}): {self.lib.cf_last_error(None).decode()}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(self.lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TimeAverager(_ChildHandle):
    """cf_average_*: after collections of weights w₁ … wₙ every `means[k]` holds Σ w f / Σ w of `sources[k]` on the interior
    (halos untouched), accumulated on the device in one launch per collection.  The library borrows the pointers: the tensors
    are kept alive here."""
    _destroy = "cf_average_destroy"

    def __init__(self, ctx, sources, means):
        self._adopt(ctx)
        self.sources, self.means = list(sources), list(means)
        if len(self.sources) != len(self.means):
            raise ValueError(f"{len(self.sources)} sources, {len(self.means)} means")
        for t in self.sources + self.means:
            if not _is_field(t, ctx):
                raise ValueError(f"averaged fields are contiguous float64 device arrays of shape {ctx.shape}")
        n = len(self.sources)
        src = (C.c_void_p * n)(*[t.data_ptr() for t in self.sources])
        dst = (C.c_void_p * n)(*[t.data_ptr() for t in self.means])
        ctx._check(self.lib.cf_average_create(ctx._h, n, src, dst, C.byref(self._h)), "cf_average_create")

    @classmethod
    def derived(cls, ctx, terms, cos_rotation=None, sin_rotation=None, max_workgroups=0):
        """cf_average_create_derived (FluxContext.derived_average): `sources` are the distinct input fields, rotation
        arrays included, `terms` the table as given."""
        self = cls.__new__(cls)
        self._adopt(ctx)
        self.terms = [tuple(t) for t in terms]
        if len(self.terms) > abi.AVERAGE_MAX_FIELDS:
            raise ValueError(f"{len(self.terms)} terms (at most {abi.AVERAGE_MAX_FIELDS})")
        table = (abi.AverageTerm * max(len(self.terms), 1))()
        self.sources, self.means = [], []

        def pointer(t, what):
            if t is None:
                return None
            if not _is_field(t, ctx):
                raise ValueError(f"{what} is a contiguous float64 device array of shape {ctx.shape}")
            if what != "mean" and not any(t is s for s in self.sources):
                self.sources.append(t)
            return t.data_ptr()
        for k, (kind, a, b, scale, flags, mean) in enumerate(self.terms):
            T = table[k]
            T.kind = TERM_KINDS[kind] if isinstance(kind, str) else int(kind)
            T.flags, T.scale = int(flags), float(scale)
            T.a, T.b, T.mean = pointer(a, f"term {k}: a"), pointer(b, f"term {k}: b"), pointer(mean, "mean")
            self.means.append(mean)
        desc = abi.AverageDesc(C.sizeof(abi.AverageDesc), len(self.terms), table, pointer(cos_rotation, "cos_rotation"),
                               pointer(sin_rotation, "sin_rotation"), int(max_workgroups), 0)
        ctx._check(self.lib.cf_average_create_derived(ctx._h, C.byref(desc), C.byref(self._h)), "cf_average_create_derived")
        return self

    @classmethod
    def budget(cls, ctx, terms, ocean=None, atmos=None, fluxes=None, ice=None, frazil_heat=None, land_freshwater=None, weights=None,
               max_workgroups=0):
        """cf_average_create_budget (FluxContext.budget_average): `sources` are the input fields given, `terms` the table."""
        self = cls.__new__(cls)
        self._adopt(ctx)
        self.terms = [tuple(t) for t in terms]
        if len(self.terms) > abi.AVERAGE_MAX_FIELDS:
            raise ValueError(f"{len(self.terms)} terms (at most {abi.AVERAGE_MAX_FIELDS})")
        table = (abi.BudgetTerm * max(len(self.terms), 1))()
        self.means = []
        for k, (kind, scale, mean) in enumerate(self.terms):
            if not _is_field(mean, ctx):
                raise ValueError(f"term {k}: the mean is a contiguous float64 device array of shape {ctx.shape}")
            table[k] = abi.BudgetTerm(BUDGET_KINDS[kind] if isinstance(kind, str) else int(kind), 0, float(scale), mean.data_ptr())
            self.means.append(mean)
        o = ctx.ocean_struct(ocean) if ocean is not None else None
        e = ctx.exchange_struct(atmos) if atmos is not None else None
        f = ctx.fluxes_struct(fluxes) if fluxes is not None else None
        i = ctx.ice_struct(ice)
        w = ctx.weights_struct(weights) if weights is not None else None
        self.sources = [t for d in (ocean, atmos, fluxes, ice, weights) if d is not None for t in d.values() if isinstance(t, torch.Tensor)]
        self.sources += [t for t in (frazil_heat, land_freshwater) if t is not None]
        ref = lambda x: C.pointer(x) if x is not None else None  # noqa: E731
        desc = abi.BudgetDesc(C.sizeof(abi.BudgetDesc), len(self.terms), table, ref(o), ref(e), ref(f), ref(i), _ptr(frazil_heat),
                              _ptr(land_freshwater), ref(w), int(max_workgroups), 0)
        ctx._check(self.lib.cf_average_create_budget(ctx._h, C.byref(desc), C.byref(self._h)), "cf_average_create_budget")
        return self

    def collect(self, weight):
        self._check(self.lib.cf_average_collect(self._h, float(weight)), "cf_average_collect")

    def reset(self):
        self._check(self.lib.cf_average_reset(self._h), "cf_average_reset")

    def weight(self):
        """(total weight, collections) of the current window."""
        total, samples = C.c_double(), C.c_int64()
        self._check(self.lib.cf_average_weight(self._h, C.byref(total), C.byref(samples)), "cf_average_weight")
        return total.value, samples.value


class _SeriesHandle(_ChildHandle):
    """What SurfaceIntegrator and SurfaceMonitor share: a series of records [n_entries] of `_dtype` kept on the device behind
    the entry points cf_<_family>_collect, _count, _read, _reset and _destroy."""
    _family = None
    _dtype = None

    def _call(self, name, *args):
        what = f"cf_{self._family}_{name}"
        self._check(getattr(self.lib, what)(self._h, *args), what)

    def collect(self, time=0.0):
        self._call("collect", float(time))

    def count(self):
        n = C.c_int64()
        self._call("count", C.byref(n))
        return n.value

    def read(self, first=0, n=None):
        """(values[n, n_entries] of the family's record type, times[n]) of records first … first + n − 1 (n = None: to the end
        of the series)."""
        n = self.count() - first if n is None else n
        values, times = np.zeros((max(n, 0), self.n_entries), dtype=self._dtype), np.zeros(max(n, 0))
        self._call("read", int(first), int(n), values.ctypes.data, times.ctypes.data_as(abi.c_double_p))
        return values, times

    def reset(self):
        self._call("reset")


INTEGRAND_KINDS = dict(one=abi.INTEGRAND_ONE, field=abi.INTEGRAND_FIELD, product=abi.INTEGRAND_PRODUCT, above=abi.INTEGRAND_ABOVE)


class SurfaceIntegrator(_SeriesHandle):
    """cf_integrals_*: every collect(time) appends one record — entry e is Σ A·x over the wet interior cells that carry the
    entry's region bit — to a series kept on the device, in one pass over the interior; read() is the only host
    synchronisation.  The library borrows the pointers: the tensors are kept alive here."""
    _destroy, _family, _dtype = "cf_integrals_destroy", "integrals", np.float64

    def __init__(self, ctx, entries, area=None, mask=None, region=None, capacity=1024, max_workgroups=0):
        self._adopt(ctx)
        self.n_entries, self.capacity = len(entries), int(capacity)
        if self.n_entries > abi.INTEGRALS_MAX_ENTRIES:
            raise ValueError(f"{self.n_entries} entries (at most {abi.INTEGRALS_MAX_ENTRIES})")
        desc = abi.IntegralsDesc()
        desc.struct_size, desc.n_entries, desc.max_workgroups = C.sizeof(abi.IntegralsDesc), self.n_entries, int(max_workgroups)
        self._keep = [area, mask, region]
        for name, t, dtype in (("area", area, torch.float64), ("mask", mask, None), ("region", region, torch.uint8)):
            if t is None:
                continue
            if not _is_field(t, ctx, dtype):
                raise ValueError(f"{name} is a contiguous device array of shape {ctx.shape}" + (f" and dtype {dtype}" if dtype else ""))
            setattr(desc, name, t.data_ptr())
        for e, entry in enumerate(entries):
            kind, a, b, threshold, bit = tuple(entry) + ("one", None, None, 0.0, 0)[len(entry):]
            E = desc.entries[e]
            E.kind = INTEGRAND_KINDS[kind] if isinstance(kind, str) else int(kind)
            E.region_bit, E.threshold = int(bit), float(threshold)
            for key, t in (("a", a), ("b", b)):
                if t is None:
                    continue
                if not _is_field(t, ctx):
                    raise ValueError(f"entry {e}: {key} is a contiguous float64 device array of shape {ctx.shape}")
                setattr(E, key, t.data_ptr())
                self._keep.append(t)
        ctx._check(self.lib.cf_integrals_create(ctx._h, C.byref(desc), self.capacity, C.byref(self._h)), "cf_integrals_create")


MONITOR_KINDS = dict(value=abi.MONITOR_VALUE, abs=abi.MONITOR_ABS)


class SurfaceMonitor(_SeriesHandle):
    """cf_monitor_*: every collect(time) appends one record — per entry the minimum and maximum over the wet interior cells
    that are not NaN with the smallest cell index of each, the counts of NaN and ±Inf wet cells with the first of them, and a
    64-bit hash of all interior cells — to a series kept on the device; read() and status() are the only host
    synchronisations.  The library borrows the pointers: the tensors are kept alive here."""
    _destroy, _family, _dtype = "cf_monitor_destroy", "monitor", abi.MONITOR_VALUE_DTYPE

    def __init__(self, ctx, entries, mask=None, first_cell=0, capacity=1024, max_workgroups=0, row_length=0):
        self._adopt(ctx)
        entries = [tuple(e) if isinstance(e, (tuple, list)) else (e, "value") for e in entries]
        self.n_entries, self.capacity, self.first_cell = len(entries), int(capacity), int(first_cell)
        self.row_length = int(row_length)   # as given: 0 stands for the context's nx
        if self.n_entries > abi.MONITOR_MAX_ENTRIES:
            raise ValueError(f"{self.n_entries} entries (at most {abi.MONITOR_MAX_ENTRIES})")
        desc = abi.MonitorDesc()
        desc.struct_size, desc.n_entries, desc.max_workgroups = C.sizeof(abi.MonitorDesc), self.n_entries, int(max_workgroups)
        desc.first_cell, desc.row_length = self.first_cell, self.row_length
        self._keep = [mask]
        if mask is not None:
            if not _is_field(mask, ctx, None):
                raise ValueError(f"mask is a contiguous device array of shape {ctx.shape}")
            desc.mask = mask.data_ptr()
        for e, (a, kind) in enumerate(entries):
            E = desc.entries[e]
            E.kind = MONITOR_KINDS[kind] if isinstance(kind, str) else int(kind)
            if a is not None:
                if not _is_field(a, ctx):
                    raise ValueError(f"entry {e}: a is a contiguous float64 device array of shape {ctx.shape}")
                E.a = a.data_ptr()
                self._keep.append(a)
        ctx._check(self.lib.cf_monitor_create(ctx._h, C.byref(desc), self.capacity, C.byref(self._h)), "cf_monitor_create")

    def status(self):
        """(index of the first record since the last reset with a non-finite wet cell, bit mask of the entries that had one in
        it); (−1, 0) when every record is clean.  Synchronises the stream and reads 16 bytes."""
        first, entries = C.c_int64(), C.c_uint32()
        self._check(self.lib.cf_monitor_status(self._h, C.byref(first), C.byref(entries)), "cf_monitor_status")
        return first.value, entries.value


def calendar_bin(table, time):
    """The bin of `time` [s] in the calendar table (edges, bin_of_interval): cf_calendar_bin, a pure host function — the time
    is rounded to the nearest second first, ties to even.  −1: not collected; ValueError outside the table or for a bad table."""
    lib = abi.load_library()
    edges = np.ascontiguousarray(table[0], dtype=np.float64)
    bin_of_interval = np.ascontiguousarray(table[1], dtype=np.int32)
    if edges.ndim != 1 or bin_of_interval.shape != (max(edges.size - 1, 0),):
        raise ValueError(f"calendar_bin: {edges.size} edges bound {edges.size - 1} intervals, got {bin_of_interval.shape}")
    out = C.c_int32(-2)
    rc = lib.cf_calendar_bin(edges.ctypes.data_as(abi.c_double_p), bin_of_interval.ctypes.data_as(abi.c_int32_p), int(edges.size),
                             float(time), C.byref(out))
    if rc != 0:
        raise ValueError(lib.cf_last_error(None).decode())
    return out.value


class Climatology(_ChildHandle):
    """cf_climatology_*: after collections (bin, weight) every `totals[k]` holds Σ w f / Σ w of `sources[k]` over all of them
    and bin b of `bins[k]` the same over the collections into b, on the interior (halos and every other bin untouched) — bit
    for bit what TimeAveragers fed those subsequences hold, in one launch per collection.  The library borrows the pointers:
    the tensors are kept alive here."""
    _destroy = "cf_climatology_destroy"

    def __init__(self, ctx, sources, totals, bins, n_bins, max_workgroups=0):
        self._adopt(ctx)
        self.sources, self.bins, self.n_bins = list(sources), list(bins), int(n_bins)
        self.totals = list(totals) if totals is not None else [None] * len(self.sources)
        n = self.n_fields = len(self.sources)
        if len(self.totals) != n or len(self.bins) != n:
            raise ValueError(f"{n} sources, {len(self.totals)} totals, {len(self.bins)} bin blocks")
        if n > abi.CLIMATOLOGY_MAX_FIELDS:
            raise ValueError(f"{n} fields (at most {abi.CLIMATOLOGY_MAX_FIELDS})")
        for t in self.sources + [t for t in self.totals if t is not None]:
            if not _is_field(t, ctx):
                raise ValueError(f"sources and totals are contiguous float64 device arrays of shape {ctx.shape}")
        for t in self.bins:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                    and tuple(t.shape) == (self.n_bins,) + tuple(ctx.shape)):
                raise ValueError(f"a bin block is a contiguous float64 device array of shape {(self.n_bins,) + tuple(ctx.shape)}")
        desc = abi.ClimatologyDesc()
        desc.struct_size, desc.n_fields, desc.n_bins, desc.max_workgroups = C.sizeof(abi.ClimatologyDesc), n, self.n_bins, int(max_workgroups)
        for k in range(n):
            desc.sources[k], desc.bins[k] = self.sources[k].data_ptr(), self.bins[k].data_ptr()
            desc.totals[k] = self.totals[k].data_ptr() if self.totals[k] is not None else None
        ctx._check(self.lib.cf_climatology_create(ctx._h, C.byref(desc), C.byref(self._h)), "cf_climatology_create")

    def collect(self, bin, weight):
        """One launch: the sources enter the totals and bin `bin` with `weight`; bin −1: nothing is collected."""
        self._check(self.lib.cf_climatology_collect(self._h, int(bin), float(weight)), "cf_climatology_collect")

    def reset(self):
        self._check(self.lib.cf_climatology_reset(self._h), "cf_climatology_reset")

    def weights(self):
        """(total weight, collections, per-bin weights [n_bins], per-bin collections [n_bins]) since the last reset."""
        total, samples = C.c_double(), C.c_int64()
        bin_totals, bin_samples = np.zeros(self.n_bins), np.zeros(self.n_bins, dtype=np.int64)
        self._check(self.lib.cf_climatology_weights(self._h, C.byref(total), C.byref(samples), bin_totals.ctypes.data_as(abi.c_double_p),
                                                    bin_samples.ctypes.data_as(C.POINTER(C.c_int64))), "cf_climatology_weights")
        return total.value, samples.value, bin_totals, bin_samples

    def extremes(self, field=0, minimum=True, maximum=True, argmin=True, argmax=True, out=None):
        """(min, max, argmin, argmax) over the non-empty bins of field `field`, per interior cell, with Julia's min / max (a NaN
        in any non-empty bin gives NaN, −0.0 < +0.0); the arg arrays (int32) hold the smallest bin that attains the result.
        Ocean-grid device arrays whose halos are left as they were — zero in a fresh one; `out`: four arrays (or None) to
        write instead.  An output whose flag is False is not computed and returned as None.  One launch."""
        ctx = self.ctx
        given = list(out) if out is not None else [None] * 4
        made = []
        for k, (want, dtype) in enumerate(((minimum, torch.float64), (maximum, torch.float64), (argmin, torch.int32), (argmax, torch.int32))):
            t = given[k] if want else None
            if want and t is None:
                t = torch.zeros(ctx.shape, dtype=dtype, device=self.sources[0].device)
            if t is not None and not _is_field(t, ctx, dtype):
                raise ValueError(f"extremes: output {k} is a contiguous {dtype} device array of shape {ctx.shape}")
            made.append(t)
        self._check(self.lib.cf_climatology_extremes(self._h, int(field), *[_ptr(t) for t in made]), "cf_climatology_extremes")
        return tuple(made)


def dataset_time_index(times, period, time):
    """(level1, level2, fraction) of `time` in a dataset's level times: cf_dataset_time_index, a pure host function — cyclical
    over `period` when it is > 0, clamped when 0.  ValueError for a time that is not finite or a bad table."""
    lib = abi.load_library()
    times = np.ascontiguousarray(times, dtype=np.float64)
    if times.ndim != 1:
        raise ValueError("dataset_time_index: times is one-dimensional")
    l1, l2, f = C.c_int32(-1), C.c_int32(-1), C.c_double(float("nan"))
    rc = lib.cf_dataset_time_index(times.ctypes.data_as(abi.c_double_p), int(times.size), float(period), float(time), C.byref(l1),
                                   C.byref(l2), C.byref(f))
    if rc != 0:
        raise ValueError(lib.cf_last_error(None).decode())
    return l1.value, l2.value, f.value


class Dataset(_ChildHandle):
    """cf_dataset_*: a dataset on its own latitude–longitude grid, staged level by level — stage(level, plane) converts a host
    float32 plane (NaN = missing) to f64, inpaints it by nearest-neighbour sweeps whose number the host knows beforehand, and
    interpolates it onto the level's ocean-grid array — and followed in time by evaluate(time), materialize_dataset_restoring
    and the coupled loop (FluxContext.attach_restoring_dataset).  The library borrows the weights: the tensors are kept here."""
    _destroy = "cf_dataset_destroy"

    def __init__(self, ctx, ns_x, ns_y, times, weights, period=0.0, periodic_x=True, max_sweeps=-1, fill_value=0.0, sweeps_per_launch=0,
                 max_workgroups=0):
        self._adopt(ctx)
        self.ns_x, self.ns_y, self.period = int(ns_x), int(ns_y), float(period)
        self.times = np.ascontiguousarray(times, dtype=np.float64)
        if self.times.ndim != 1:
            raise ValueError("times is one-dimensional")
        self.n_levels = int(self.times.size)
        self._keep = weights
        desc = abi.DatasetDesc()
        desc.struct_size = C.sizeof(abi.DatasetDesc)
        desc.ns_x, desc.ns_y, desc.n_levels, desc.periodic_x = self.ns_x, self.ns_y, self.n_levels, 1 if periodic_x else 0
        desc.max_sweeps, desc.sweeps_per_launch, desc.max_workgroups = int(max_sweeps), int(sweeps_per_launch), int(max_workgroups)
        desc.fill_value, desc.period, desc.times = float(fill_value), self.period, self.times.ctypes.data
        desc.weights = ctx.weights_struct(weights)
        ctx._check(self.lib.cf_dataset_create(ctx._h, C.byref(desc), C.byref(self._h)), "cf_dataset_create")

    def stage(self, level, plane):
        """Queue the staging of `plane` (host array [ns_y, ns_x], NaN = missing) as level `level`; no synchronisation."""
        plane = np.ascontiguousarray(plane, dtype=np.float32)
        if plane.shape != (self.ns_y, self.ns_x):
            raise ValueError(f"stage: the plane is [{self.ns_y}, {self.ns_x}], got {plane.shape}")
        self._check(self.lib.cf_dataset_stage(self._h, int(level), plane.ctypes.data), "cf_dataset_stage")

    def level(self, level):
        """A copy of the level's ocean-grid array as a device tensor (synchronises; level_pointer gives the borrowed address)."""
        host = np.empty(self.ctx.shape, dtype=np.float64)
        self.ctx._check(self.lib.cf_d2h(self.ctx._h, host.ctypes.data, self.level_pointer(level), host.nbytes), "cf_d2h")
        return torch.from_numpy(host).to(self.ctx.device)

    def level_pointer(self, level):
        """The device address of the level's ocean-grid array, borrowed from the dataset (cf_dataset_level)."""
        p = C.c_void_p()
        self._check(self.lib.cf_dataset_level(self._h, int(level), C.byref(p)), "cf_dataset_level")
        return p.value

    def read_source(self):
        """The inpainted f64 plane [ns_y, ns_x] of the most recently staged level; synchronises."""
        out = np.empty((self.ns_y, self.ns_x), dtype=np.float64)
        self._check(self.lib.cf_dataset_read_source(self._h, out.ctypes.data), "cf_dataset_read_source")
        return out

    def stage_info(self, level):
        """(sweeps queued, cells filled by a sweep, cells given the fill value) of a staged level: host bookkeeping."""
        sweeps, filled, defaulted = C.c_int32(), C.c_int64(), C.c_int64()
        self._check(self.lib.cf_dataset_stage_info(self._h, int(level), C.byref(sweeps), C.byref(filled), C.byref(defaulted)),
                    "cf_dataset_stage_info")
        return sweeps.value, filled.value, defaulted.value

    def time_index(self, time):
        return dataset_time_index(self.times, self.period, time)

    def evaluate(self, time, out):
        """S★ at `time` on the ring window of `out` (an ocean-grid float64 field); one launch."""
        if not _is_field(out, self.ctx):
            raise ValueError(f"evaluate: out is a contiguous float64 device array of shape {self.ctx.shape}")
        self._check(self.lib.cf_dataset_evaluate(self._h, float(time), _ptr(out)), "cf_dataset_evaluate")
        return out


def _host_bytes(data):
    """(keep-alive object, address, length) of a bytes-like object, without copying where it is writable or bytes."""
    if isinstance(data, bytes):
        return data, C.cast(C.c_char_p(data), C.c_void_p), len(data)
    a = np.frombuffer(data, dtype=np.uint8)
    if not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    return a, C.c_void_p(a.ctypes.data), a.size


def checkpoint_hash(data):
    """The section hash of a checkpoint image over `data` (bytes-like): cf_checkpoint_hash, a pure host function —
    Σ mix64(w_k XOR K·(k + 1)) mod 2⁶⁴ over the 8-byte little-endian words, the last one zero padded."""
    lib = abi.load_library()
    keep, p, n = _host_bytes(data)
    out = C.c_uint64()
    if lib.cf_checkpoint_hash(p, n, C.byref(out)) != 0:
        raise ValueError(lib.cf_last_error(None).decode())
    return out.value


def checkpoint_verify(image):
    """Checks a checkpoint image (bytes-like) without a device: cf_checkpoint_verify.  ValueError names the header field or
    the section that is wrong."""
    lib = abi.load_library()
    keep, p, n = _host_bytes(image)
    if lib.cf_checkpoint_verify(p, n) != 0:
        raise ValueError(lib.cf_last_error(None).decode())


def checkpoint_host_blob(image):
    """The caller's blob inside a checkpoint image (cf_checkpoint_host_blob; the image is verified first)."""
    lib = abi.load_library()
    keep, p, n = _host_bytes(image)
    blob, size = C.c_void_p(), C.c_size_t()
    if lib.cf_checkpoint_host_blob(p, n, C.byref(blob), C.byref(size)) != 0:
        raise ValueError(lib.cf_last_error(None).decode())
    return C.string_at(blob.value, size.value) if size.value else b""


class Checkpoint(_ChildHandle):
    """cf_checkpoint_*: packs registered device arrays and the private state of TimeAveragers, Climatologies,
    SurfaceIntegrators and SurfaceMonitors into one self-describing image (this library's own format, not JLD2) and puts such
    an image back, bit for bit.  capture() is stream ordered and returns at once — one launch packs and hashes every section,
    the image drains on the handle's own stream while later steps run; wait() returns the finished image; restore(image)
    refuses whatever does not match the registration before it writes a byte.  `direct`: no device staging image (sections
    are copied one by one on the context's stream).  The library borrows arrays and handles: they are kept alive here."""
    _destroy = "cf_checkpoint_destroy"

    def __init__(self, ctx, direct=False, max_workgroups=0):
        self._adopt(ctx)
        self.names, self._keep = [], []
        flags = abi.CHECKPOINT_DIRECT if direct else 0
        desc = abi.CheckpointDesc(C.sizeof(abi.CheckpointDesc), flags, int(max_workgroups), 0)
        ctx._check(self.lib.cf_checkpoint_create(ctx._h, C.byref(desc), C.byref(self._h)), "cf_checkpoint_create")

    def add_array(self, name, tensor):
        """A contiguous device tensor of any dtype (a whole parent array, a [k] slab of one): all its bytes."""
        if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.is_contiguous()):
            raise ValueError(f"section {name!r}: a contiguous device tensor")
        self._check(self.lib.cf_checkpoint_add_array(self._h, name.encode(), C.c_void_p(tensor.data_ptr()), tensor.numel() * tensor.element_size()),
                    "cf_checkpoint_add_array")
        self.names.append(name)
        self._keep.append(tensor)

    def add(self, name, handle):
        """The library-private state of a TimeAverager, Climatology, SurfaceIntegrator or SurfaceMonitor of the same context
        (its weights, counts, times, records, status); the arrays it writes into are registered with add_array."""
        for cls, kind in ((TimeAverager, "average"), (Climatology, "climatology"), (SurfaceIntegrator, "integrals"), (SurfaceMonitor, "monitor")):
            if isinstance(handle, cls):
                what = "cf_checkpoint_add_" + kind
                self._check(getattr(self.lib, what)(self._h, name.encode(), handle._h), what)
                self.names.append(name)
                self._keep.append(handle)
                return
        raise ValueError(f"section {name!r}: {type(handle).__name__} has no state a checkpoint keeps")

    def set_host_blob(self, data):
        keep, p, n = _host_bytes(data)
        self._check(self.lib.cf_checkpoint_set_host_blob(self._h, p, n), "cf_checkpoint_set_host_blob")

    def capture(self):
        self._check(self.lib.cf_checkpoint_capture(self._h), "cf_checkpoint_capture")

    def wait(self, copy=True):
        """Waits for the drain of the last capture (and for the check of the last restore) and returns the image: bytes, or
        with copy=False a memoryview of the library's pinned buffer, valid until the next capture, restore or close.  None when
        nothing was captured."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self.lib.cf_checkpoint_wait(self._h, C.byref(p), C.byref(n)), "cf_checkpoint_wait")
        if not p.value:
            return None
        return C.string_at(p.value, n.value) if copy else memoryview((C.c_ubyte * n.value).from_address(p.value)).cast("B")

    def restore(self, image):
        keep, p, n = _host_bytes(image)
        self._check(self.lib.cf_checkpoint_restore(self._h, p, n), "cf_checkpoint_restore")


REGRID_MODES = dict(mean=abi.REGRID_MEAN, sum=abi.REGRID_SUM)


class SurfaceRegridder(_ChildHandle):
    """cf_regrid_*: apply(sources) → one dense device tensor of n_rows doubles per source, dst[r] = Σ w x / Σ w over the wet
    entries of row r ("mean"; NaN where no entry is wet) or Σ w x ("sum"), and `coverage` = Σ w — one pass for all sources, no
    host synchronisation.  The operator is copied to the device at construction; the mask is borrowed and kept alive here."""
    _destroy = "cf_regrid_destroy"

    def __init__(self, ctx, row_ptr, col, weight, mask=None, mode="mean", max_workgroups=0):
        self._adopt(ctx)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        weight = np.ascontiguousarray(weight, dtype=np.float64)
        if row_ptr.ndim != 1 or row_ptr.size < 2 or col.ndim != 1 or col.shape != weight.shape:
            raise ValueError("regridder: row_ptr (n_rows + 1 entries, n_rows ≥ 1), col and weight (nnz entries each) are 1-D arrays")
        if mask is not None and not _is_field(mask, ctx, None):
            raise ValueError(f"mask is a contiguous device array of shape {ctx.shape}")
        self.n_rows, self.nnz, self.mask = row_ptr.size - 1, col.size, mask
        self.mode = REGRID_MODES[mode] if isinstance(mode, str) else int(mode)
        desc = abi.RegridDesc()
        desc.struct_size, desc.mode, desc.n_rows, desc.nnz = C.sizeof(abi.RegridDesc), self.mode, self.n_rows, self.nnz
        desc.row_ptr, desc.col, desc.weight = row_ptr.ctypes.data, col.ctypes.data, weight.ctypes.data
        desc.mask, desc.max_workgroups = (mask.data_ptr() if mask is not None else None), int(max_workgroups)
        ctx._check(self.lib.cf_regrid_create(ctx._h, C.byref(desc), C.byref(self._h)), "cf_regrid_create")
        self.coverage = None

    def apply(self, sources, out=None, coverage=True):
        """Regrids `sources` (ocean-grid float64 device fields) into `out` (device tensors of at least n_rows doubles; new ones
        by default) and returns them; `self.coverage` is the row sums of the wet weights (coverage=False: not written, None;
        a tensor: written there)."""
        sources = list(sources)
        for t in sources:
            if not _is_field(t, self.ctx):
                raise ValueError(f"regridded fields are contiguous float64 device arrays of shape {self.ctx.shape}")
        n = len(sources)
        if out is None:
            out = [torch.empty(self.n_rows, dtype=torch.float64, device=self.ctx.device) for _ in sources]
        out = list(out)
        if len(out) != n:
            raise ValueError(f"{n} sources, {len(out)} outputs")
        if coverage is True:
            coverage = torch.empty(self.n_rows, dtype=torch.float64, device=self.ctx.device)
        elif coverage is False:
            coverage = None
        for t in out + ([coverage] if coverage is not None else []):
            if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float64 and t.numel() >= self.n_rows):
                raise ValueError(f"outputs are contiguous float64 device arrays of at least {self.n_rows} elements")
        src = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in sources])
        dst = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in out])
        self._check(self.lib.cf_regrid_apply(self._h, n, src, dst, _ptr(coverage)), "cf_regrid_apply")
        self.coverage = coverage
        return out


class SnapshotWindow(_ChildHandle):
    """JRA55PrescribedAtmosphere(arch; time_indices_in_memory = n_slots, prefetch = true): cf_window_* —
    `n_slots` snapshots of the nine JRA55 variables in HBM, refilled asynchronously from pinned staging
    buffers on a copy stream (atmosphere.jl:20-29).  Snapshot t lives in slot t mod n_slots."""
    _destroy = "cf_window_destroy"

    def __init__(self, ctx, ns_x, ns_y, n_slots):
        self._adopt(ctx)
        self.ns_x, self.ns_y, self.n_slots = ns_x, ns_y, n_slots
        ctx._check(self.lib.cf_window_create(ctx._h, ns_x, ns_y, n_slots, C.byref(self._h)), "cf_window_create")

    def host_view(self, slot, variable):
        """NumPy view (ns_y, ns_x) float32 of the pinned staging buffer of (slot, variable)."""
        k = abi.JRA55_VARIABLES.index(variable) if isinstance(variable, str) else variable
        p = self.lib.cf_window_host_buffer(self._h, slot, k)
        if not p:
            raise CofluxError(f"no staging buffer for slot {slot}, variable {variable}")
        return np.ctypeslib.as_array(p, shape=(self.ns_y, self.ns_x))

    def wait_slot(self, slot):
        self._check(self.lib.cf_window_wait_slot(self._h, slot), "cf_window_wait_slot")

    def commit(self, slot, time_index):
        self._check(self.lib.cf_window_commit(self._h, slot, time_index), "cf_window_commit")

    def upload(self, time_index, snapshot):
        """snapshot: dict variable -> float32 (ns_y, ns_x) host array."""
        keep = [np.ascontiguousarray(snapshot[v], dtype=np.float32) for v in abi.JRA55_VARIABLES]
        for a in keep:
            assert a.shape == (self.ns_y, self.ns_x), a.shape
        ptrs = (C.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
        self._check(self.lib.cf_window_upload(self._h, time_index, ptrs), "cf_window_upload")

    def find(self, time_index):
        return self.lib.cf_window_find(self._h, time_index)

    def source(self, n1, n2, time_fraction):
        s = abi.AtmosSource()
        self._check(self.lib.cf_window_source(self._h, n1, n2, float(time_fraction), C.byref(s)), "cf_window_source")
        return s


def comm_unique_id():
    lib = abi.load_library()
    buf = C.create_string_buffer(abi.COMM_ID_BYTES)
    rc = lib.cf_comm_unique_id(buf)
    if rc != 0:
        raise CofluxError(f"cf_comm_unique_id failed: {lib.cf_last_error(None).decode()}")
    return buf.raw
