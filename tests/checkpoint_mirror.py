"""The mirror's pickup case (tests/test_checkpoint.py): the 48 × 24 model of tests/test_coupled_steps.py — sea ice,
JRA55PrescribedLand, a SurfaceFluxRestoring on S, NormalizeSalinity as a callback — under run!(simulation) with four writers
and a Checkpointer, and everything a run leaves behind as one dict of host arrays.  Run as a program it is the SECOND process
of a split run:  python checkpoint_mirror.py <dir> <out.npz> <dt> [<dt> …]  picks up in <dir>/<dt> and runs to iteration 12."""
import datetime
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "climaocean.jl_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

N_ITERATIONS, SPLIT = 12, 5
# the month turns at t = 3 h: iteration 8 of Δt = 3 h / 8, iteration 9 of Δt = 20 min — after the split either way
REFERENCE_DATE = datetime.datetime(1958, 1, 31, 21)


def simulation(dt, directory, stop_iteration):
    import test_coupled_steps as tcs
    from coflux import models as cm
    model, normalize = tcs._model()
    itf = model.interfaces
    sim = cm.Simulation(model, dt=dt, stop_iteration=stop_iteration)
    net = itf.net_fluxes._ocean_fields
    sim.output_writers["surface"] = cm.SurfaceFluxAverages(model, schedule=cm.AveragedTimeInterval(4 * dt))   # windows end at 4, 8, 12
    sim.output_writers["monthly"] = cm.MonthlyClimatology(model, {"hfds": net["T"], "sic": model.sea_ice.concentration}, reference_date=REFERENCE_DATE)
    sim.output_writers["ice"] = cm.sea_ice_integrals(model)
    sim.output_writers["extrema"] = cm.SurfaceExtrema(model, {"hfds": net["T"], "tauuo": (net["u"], "abs"), "Ts": model.sea_ice.top_surface_temperature})
    sim.output_writers["checkpoint"] = cm.Checkpointer(model, schedule=cm.IterationInterval(SPLIT), dir=directory)
    cm.add_callback(sim, normalize, name="normalize")
    return sim, normalize


def results(sim, normalize):
    """Every field of the model, the windows, both series with their times, the climatology and the clocks, as host arrays."""
    import test_coupled_steps as tcs
    m = sim.model
    m.interfaces.context.sync()
    out = {"field." + k: v.detach().cpu().numpy().view(np.int64) for k, v in tcs._model_fields(m, normalize).items()}
    out["clock"] = np.array([m.clock.time, m.clock.iteration, m.ocean.model.clock.time, m.ocean.model.clock.iteration])
    w = sim.output_writers
    for t_k, arrays in w["surface"].windows:
        for name, a in arrays.items():
            out[f"window.{t_k!r}.{name}"] = a.view(np.int64)
    out["average_weight"] = np.array(w["surface"].averager.weight())
    for name in ("ice", "extrema"):
        values, times = w[name].records()
        out[f"{name}.values"] = np.frombuffer(values.tobytes(), dtype=np.uint8)
        out[f"{name}.times"] = times.copy()
    out["extrema.status"] = np.array(w["extrema"].monitor.status())
    clim = w["monthly"]
    total, samples, bw, bs = clim.climatology.weights()
    out["monthly.weights"] = np.concatenate([[total, samples], bw, bs])
    for name in clim.names:
        out[f"monthly.total.{name}"] = clim.totals[name].cpu().numpy().view(np.int64)
        out[f"monthly.bins.{name}"] = clim.bins[name].cpu().numpy().view(np.int64)
    return out


def main(argv):
    from coflux import models as cm
    root, out_path, dts = argv[0], argv[1], [float(x) for x in argv[2:]]
    everything = {}
    for dt in dts:
        sim, normalize = simulation(dt, os.path.join(root, repr(dt)), N_ITERATIONS)
        cm.run(sim, pickup=True)
        assert sim.model.clock.iteration == N_ITERATIONS
        everything.update({f"{dt!r}/{k}": v for k, v in results(sim, normalize).items()})
        sim.output_writers["checkpoint"].close()
    np.savez(out_path, **everything)


if __name__ == "__main__":
    main(sys.argv[1:])
