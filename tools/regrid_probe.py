"""Cost of the sparse surface operator on the 1/4-degree surface (1440 x 560, halo 7, synthetic mask) -> profiles/regrid_probe.json.

    python tools/regrid_probe.py [--applies N] [--rounds R] [--out PATH]

The driver starts the GPU step as a child under its own `timeout`; nothing follows a step that failed.  The child, one
process, warm-up first, the arms alternating over `rounds` rounds:
  * cf_regrid_apply of the conservative map 1/4 degree -> 360 x 180 (50 400 rows of 16 entries) with K = 1, 6 and 16 fields and
    of the zonal operator (140 rows of 5 760 entries) with K = 6, HIP events over `applies` back-to-back applies;
  * cf_time_copy of each apply's algorithmic bytes, nnz (13 + 8 K) + 8 n_rows (K + 1), in the same process;
  * what a caller had before: torch.sparse CSR x dense of x * m and of m on the device fields, then the division."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "climaocean.jl_amd"))

NX, NY, H = 1440, 560, 7


def measure(applies, rounds):
    import numpy as np
    import torch
    from coflux import models as cm, regridding as rg, synthetic as syn, interface_computations as ic
    from coflux.runtime import FluxContext

    def events_ms(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    ctx = FluxContext(NX, NY, H, H, ic.flux_params(), ring=1)
    grid = cm.LatitudeLongitudeGrid(size=(NX, NY, 10), halo=(H, H, H))
    mask = ctx.to_device(syn.ocean_state(NX, NY, H, H)["mask"])
    gen = torch.Generator(device=ctx.device).manual_seed(0)
    fields = [torch.randn(ctx.shape, dtype=torch.float64, device=ctx.device, generator=gen) for _ in range(16)]
    operators = dict(map=rg.conservative_latlon_weights(grid), zonal=rg.zonal_mean_weights(grid))
    inner = (slice(H, H + NY), slice(H, H + NX))
    m_flat = (mask[inner] != 0).to(torch.float64).reshape(-1, 1).contiguous()
    arms, layouts = {}, {}
    for name, K in (("map", 1), ("map", 6), ("map", 16), ("zonal", 6)):
        op = operators[name]
        regridder = ctx.regridder(*op, mask=mask)
        src = fields[:K]
        dst = [torch.empty(op.n_rows, dtype=torch.float64, device=ctx.device) for _ in src]
        cov = torch.empty(op.n_rows, dtype=torch.float64, device=ctx.device)
        csr = torch.sparse_csr_tensor(torch.from_numpy(op.row_ptr), torch.from_numpy(op.col.astype(np.int64)),
                                      torch.from_numpy(op.weight), size=(op.n_rows, NX * NY)).to(ctx.device)
        layouts[f"{name}_K{K}"] = "csr"
        try:
            csr @ m_flat
        except RuntimeError:    # a torch build without CSR x dense on the device: the COO form a caller would then have used
            csr = csr.to_sparse_coo().coalesce()
            layouts[f"{name}_K{K}"] = "coo"

        def ours(regridder=regridder, src=src, dst=dst, cov=cov):
            regridder.apply(src, out=dst, coverage=cov)

        def torch_form(csr=csr, src=src):
            x = torch.stack([f[inner].reshape(-1) for f in src], dim=1) * m_flat    # materialises x · m
            return (csr @ x) / (csr @ m_flat)

        nbytes = op.col.size * (13 + 8 * K) + 8 * op.n_rows * (K + 1)
        arms[f"{name}_K{K}"] = dict(ours=ours, torch=torch_form, bytes=nbytes, nnz=int(op.col.size), n_rows=int(op.n_rows), fields=K,
                                    keep=(regridder, csr), t_ours=[], t_torch=[], t_copy=[])
    for arm in arms.values():       # warm-up: code load, clocks, torch's sparse set-up
        for _ in range(20):
            arm["ours"]()
            arm["torch"]()
    for _ in range(rounds):         # alternating
        for arm in arms.values():
            arm["t_ours"].append(events_ms(arm["ours"], applies))
            arm["t_copy"].append(ctx.time_copy(arm["bytes"] // 2 // 8 * 8, applies))
            arm["t_torch"].append(events_ms(arm["torch"], max(applies // 10, 20)))
    # the two arms agree (the torch form multiplies land by zero: the probe's fields are finite everywhere)
    agreement = {}
    for key, arm in arms.items():
        regridder = arm["keep"][0]
        ours = torch.stack(regridder.apply(fields[:arm["fields"]]), dim=1)
        ref = arm["torch"]()
        both = ~torch.isnan(ref)
        agreement[key] = float(((ours - ref)[both].abs() / ref[both].abs().clamp_min(1e-300)).max())
        assert bool((torch.isnan(ours) == torch.isnan(ref)).all())
    ctx.sync()
    result = dict(grid=[NX, NY, H], applies=applies, rounds=rounds, device=torch.cuda.get_device_name(0))
    for key, arm in arms.items():
        o, c, t = min(arm["t_ours"]), min(arm["t_copy"]), min(arm["t_torch"])
        result[key] = dict(nnz=arm["nnz"], n_rows=arm["n_rows"], fields=arm["fields"], algorithmic_bytes=arm["bytes"],
                           apply_us=round(1e3 * o, 2), apply_us_all=[round(1e3 * x, 2) for x in arm["t_ours"]],
                           apply_tbps=round(arm["bytes"] / (o * 1e-3) / 1e12, 3),
                           copy_same_bytes_us=round(1e3 * c, 2), copy_us_all=[round(1e3 * x, 2) for x in arm["t_copy"]],
                           copy_over_apply=round(c / o, 3), apply_over_copy=round(o / c, 2),
                           torch_us=round(1e3 * t, 2), torch_us_all=[round(1e3 * x, 2) for x in arm["t_torch"]],
                           torch_over_apply=round(t / o, 2), torch_layout=layouts[key], relative_difference_to_torch=agreement[key])
    for arm in arms.values():
        arm["keep"][0].close()
    ctx.close()
    print("REGRID_PROBE " + json.dumps(result))


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), *args]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        raise SystemExit(f"regrid_probe: step {' '.join(args)} ended with status {p.returncode}; nothing further is run")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("REGRID_PROBE ")]
    return json.loads(lines[-1][len("REGRID_PROBE "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--applies", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regrid_probe.json"))
    a = ap.parse_args()
    if a.measure:
        return measure(a.applies, a.rounds)
    result = child(["--measure", "--applies", str(a.applies), "--rounds", str(a.rounds)], 420)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
