"""What a tile world's exchange costs per step beside the latitude slabs' exchange, measured: writes
profiles/tile_exchange_probe.json (`--out` writes elsewhere) and prints it as one JSON line.

Two processes share the one device (one rank each, mailboxes through HIP IPC, gloo for the handles).  Per rank 1080 x 540 cells —
a tile of the 2160 x 1080 tripolar surface under Partition(2,2) (BASELINE config 5) —, halo 7, the four ocean fields, two rows,
ring + 1 columns.  The stand-alone entry points, CALLS exchanges per round on the context's stream between two events:
  (a) tile_columns       a (2,1) latitude-longitude world: the x-phase launch alone (no rank has a south or north side);
  (b) tile_columns_fold  a (2,1) tripolar world: the x-phase launch and the y-phase launch whose north side sends the fold to
                         the partner — the two launches a top-row rank of a Partition(2,2) run issues, less its south side,
                         which runs beside the north side in the same launch;
  (c) slab_rows          the parent's exchange, cf_halo_exchange_rows_peer, between two latitude slabs of the same 1080 x 540
                         cells: one launch, one side each.
(b) - (a) is the y-phase launch.  Reported as the median and the min ... max of the rounds' microseconds per exchange, not gated:
two ranks that time-share one device say nothing about xGMI, and the multi-device step stays unmeasured."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "climaocean.jl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

NX, NY, H = 1080, 540, 7
ROUNDS, CALLS, WARMUP = 5, 200, 50
FORMS = ("tile_columns", "tile_columns_fold", "slab_rows")
JOIN_LIMIT = 240


def summary(rounds):
    return dict(median_us=round(statistics.median(rounds), 3), min_us=round(min(rounds), 3), max_us=round(max(rounds), 3),
                rounds_us=[round(r, 3) for r in rounds])


def worker(rank, world, init, out):
    import torch.distributed as dist
    from coflux import abi, interface_computations as ic
    from coflux.distributed import SlabHaloExchanger, connect_tiles
    from coflux.runtime import FluxContext
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        result = {}
        locations, signs = [abi.FOLD_CENTER, abi.FOLD_CENTER, abi.FOLD_X_FACE, abi.FOLD_Y_FACE], [1.0, 1.0, -1.0, -1.0]
        for form in FORMS:
            ctx = FluxContext(NX, NY, H, H, ic.flux_params(), ring=1)
            fields = [ctx.zeros() for _ in range(4)]
            if form == "slab_rows":
                SlabHaloExchanger(ctx, NY, H, backend="peer")
                exchange = lambda: ctx.halo_exchange_rows_peer(fields, 2)  # noqa: E731
            else:
                fold = form == "tile_columns_fold"
                connect_tiles(ctx, 2, 1, fold)
                exchange = lambda: ctx.halo_exchange_tile_peer(fields, locations, signs, rows=2, fold_north=fold)  # noqa: E731
            rounds = []
            for n in [WARMUP] + [CALLS] * ROUNDS:
                torch.cuda.synchronize()
                dist.barrier()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(n):
                    exchange()
                b.record()
                ctx.sync()           # (a rank that never arrived raises here: nothing more is started)
                rounds.append(1e3 * a.elapsed_time(b) / n)
            result[form] = dict(summary(rounds[1:]), stats=list(ctx.tile_stats() if form != "slab_rows" else ctx.peer_halo_stats()))
            dist.barrier()
            ctx.close()
        result["y_phase_launch_us"] = round(result["tile_columns_fold"]["median_us"] - result["tile_columns"]["median_us"], 3)
        out[rank] = result
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_exchange_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tile_exchange_probe needs a HIP device: nothing is measured without one")
    import torch.multiprocessing as mp
    import util
    ctxm = mp.get_context("spawn")
    shared = ctxm.Manager().dict()
    init = util.rendezvous()
    procs = [ctxm.Process(target=worker, args=(r, 2, init, shared)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(JOIN_LIMIT)
        codes = [p.exitcode for p in procs]
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    if codes != [0, 0]:
        raise SystemExit(f"worker exit codes {codes}")
    out = dict(cells_per_rank=[NX, NY], halo=H, fields=4, rows=2, rounds=ROUNDS, exchanges_per_round=CALLS, warmup=WARMUP,
               device=torch.cuda.get_device_name(0), note="two ranks time-sharing one device: says nothing about xGMI",
               ranks={str(r): shared[r] for r in range(2)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
