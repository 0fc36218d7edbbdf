"""Latitude-slab sharding of the surface grid (the reference's own production
shapes are Partition(1,4) launch.sh:165 and Partition(1,8) pbs_launch.sh:51: contiguous j-slabs,
one rank per GPU).

The flux kernels need one halo row of the ocean surface state from each neighbour
(v[j+1] north; the ring row south/north when ring = 1).  On GPUs the rows travel over
RCCL/xGMI through libcoflux's cf_halo_exchange_rows; the torch.distributed point-to-point form
below is the same exchange for CPU tensors (gloo) and is what the world_size-2 CPU tests run.
"""
import torch
import torch.distributed as dist


def slab_bounds(ny_global, rank, world_size):
    """Rows [j0, j1) owned by `rank`: as equal as possible, remainder to the southern ranks."""
    base, rem = divmod(ny_global, world_size)
    j0 = rank * base + min(rank, rem)
    return j0, j0 + base + (1 if rank < rem else 0)


def halo_row_slices(ny, hy, rows):
    """(send_south, recv_south, send_north, recv_north) row slices of a (ny+2hy, ·) slab array."""
    return (slice(hy, hy + rows), slice(hy - rows, hy),
            slice(hy + ny - rows, hy + ny), slice(hy + ny, hy + ny + rows))


def exchange_halo_rows_torch(tensors, ny, hy, rows=1, group=None):
    """Neighbour exchange of `rows` boundary rows for every tensor in `tensors` using
    torch.distributed P2P (gloo on CPU, RCCL on GPU).  Non-periodic in j: the first and last
    ranks keep their outer halos."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    if world == 1:
        return
    ss, rs, sn, rn = halo_row_slices(ny, hy, rows)
    ops, recvs = [], []
    for t in tensors:
        if rank > 0:
            buf = torch.empty_like(t[rs])
            ops.append(dist.P2POp(dist.isend, t[ss].contiguous(), rank - 1, group))
            ops.append(dist.P2POp(dist.irecv, buf, rank - 1, group))
            recvs.append((t, rs, buf))
        if rank < world - 1:
            buf = torch.empty_like(t[rn])
            ops.append(dist.P2POp(dist.isend, t[sn].contiguous(), rank + 1, group))
            ops.append(dist.P2POp(dist.irecv, buf, rank + 1, group))
            recvs.append((t, rn, buf))
    for req in dist.batch_isend_irecv(ops):
        req.wait()
    for t, sl, buf in recvs:
        t[sl].copy_(buf)


def fold_north_halo_torch(t, nx, ny, hx, hy, rows, location="center", sign=1.0):
    """Tripolar fold of one (ny+2hy, nx+2hx) array held by the LAST slab (include/coflux.h: cf_fold_north_halo;
    Oceananigans' zipper boundary condition): north halo rows from the slab's own mirrored interior rows.
    The torch form of the fold for CPU slabs (gloo tests); libcoflux's kernel is the GPU form."""
    i = torch.arange(-hx, nx + hx) % nx
    for r in range(1, rows + 1):
        if location == "x_face":
            src_i, src_j, sg = (nx - i) % nx, ny - 1 - r, torch.where(i == 0, abs(sign), sign).to(t.dtype)
        elif location == "y_face":
            src_i, src_j, sg = nx - 1 - i, ny - r, sign
        else:
            src_i, src_j, sg = nx - 1 - i, ny - 1 - r, sign
        t[hy + ny - 1 + r, :] = sg * t[hy + src_j, hx + src_i]


class SlabHaloExchanger:
    """Per-step halo exchange of the ocean surface fields of one slab.

    backend "rccl": libcoflux's grouped ncclSend/ncclRecv on its communication stream (the unique id is
    created on rank 0 and broadcast with torch.distributed); "peer": libcoflux's peer-direct mailboxes (HIP IPC
    handles gathered with torch.distributed); "torch": torch.distributed P2P.
    `rows` defaults to ring + 1: with ring = 1 the kernels also compute row j = ny, whose cell-centre v reads the
    y-face at j = ny + 1.
    """

    def __init__(self, ctx, ny, hy, rows=None, backend="rccl"):
        self.ctx, self.ny, self.hy = ctx, ny, hy
        self.rows = rows if rows is not None else ctx.grid.ring + 1
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.backend = backend if self.world > 1 else "none"
        if self.backend == "peer":
            # cf_peer_halo_export fails (CF_ERR_COMM) on a rank whose device cannot give it fine-grained memory.  Every
            # rank reaches the collectives below whatever happened locally: the ranks agree on the outcome first, and a
            # failure anywhere moves ALL of them to the RCCL exchange together (a rank that raised before the gather
            # would leave the others blocked in it — ADVICE r3).
            mine, failure = None, None
            try:
                mine = ctx.peer_halo_export(max_fields=4, max_rows=self.rows)
            except Exception as exc:  # noqa: BLE001 — reported below, on every rank
                failure = f"rank {self.rank}: {exc}"
            handles = [None] * self.world
            dist.all_gather_object(handles, (mine, failure))
            failures = [f for _, f in handles if f is not None]
            if failures:
                self.peer_fallback_reason = "; ".join(failures)
                self.backend = "rccl"
            else:
                handles = [h for h, _ in handles]
                ctx.peer_halo_connect(handles[self.rank - 1] if self.rank > 0 else None,
                                      handles[self.rank + 1] if self.rank < self.world - 1 else None, self.rank, self.world)
        if self.backend == "rccl":
            from . import runtime
            # rank 0 always reaches the broadcast — with the id or with the reason it has none — so that no rank is left
            # waiting in it; every rank then raises the same error
            ident = [None]
            if self.rank == 0:
                try:
                    ident = [(runtime.comm_unique_id(), None)]
                except Exception as exc:  # noqa: BLE001
                    ident = [(None, f"rank 0: {exc}")]
            dist.broadcast_object_list(ident, src=0)
            uid, failure = ident[0]
            if failure is not None:
                raise RuntimeError(f"no RCCL unique id ({failure})")
            ctx.comm_init(uid, self.rank, self.world)

    def __call__(self, tensors):
        if self.backend == "rccl":
            self.ctx.halo_exchange_rows(tensors, self.rows)
        elif self.backend == "peer":
            self.ctx.halo_exchange_rows_peer(tensors, self.rows)
        elif self.backend == "torch":
            exchange_halo_rows_torch(tensors, self.ny, self.hy, self.rows)


MAX_EXCHANGE_FIELDS = 8     # PEER_MAX_FIELDS: the most fields one exchange launch carries

# What cf_time_steps_coupled exchanges under CF_HALO_PEER, in the order of include/coflux.h, and how the tripolar fold maps each
# field on the rank that owns it: (name, location, sign).  The ice velocities lie at cell centres (cf_sea_ice_state) and change
# sign across the fold like every vector component; the stresses lie on the faces of the ocean velocities.
COUPLED_STEP_FIELDS = (("T", "center", 1.0), ("S", "center", 1.0), ("u", "x_face", -1.0), ("v", "y_face", -1.0),
                       ("concentration", "center", 1.0), ("thickness", "center", 1.0), ("snow_thickness", "center", 1.0),
                       ("ice_u", "center", -1.0), ("ice_v", "center", -1.0), ("albedo", "center", 1.0))
COUPLED_CALL_FIELDS = (("x_stress", "x_face", -1.0), ("y_stress", "y_face", -1.0), ("skin_temperature", "center", 1.0))


def _cut(fields, present):
    kept = [f for f in fields if f[0] in present]
    return [kept[at:at + MAX_EXCHANGE_FIELDS] for at in range(0, len(kept), MAX_EXCHANGE_FIELDS)]


def coupled_fold_plan(ocean_present=("T", "S", "u", "v"), ice_present=("concentration", "thickness"), call_present=("skin_temperature",)):
    """The exchanges of one cf_time_steps_coupled call under CF_HALO_PEER as lists of (name, location, sign), by the C cut
    (csrc/coflux_steps.cpp: coupled_step_rows, coupled_call_rows): `per_step` — the ocean fields, then the present fields of
    the step's ice state (names of cf_sea_ice_state, its velocities as "ice_u", "ice_v") — and `per_call` — the present ones
    of x_stress, y_stress, skin_temperature —, each cut into exchanges of at most eight fields in that order.  On the rank
    that passes fold_north these triples are what the north side of each exchange folds.  Returns (per_call, per_step)."""
    step_present = set(ocean_present) | {("ice_" + k if k in ("u", "v") else k) for k in ice_present}
    return _cut(COUPLED_CALL_FIELDS, set(call_present)), _cut(COUPLED_STEP_FIELDS, step_present)


def connect_coupled_slabs(ctx, max_fields=8, rows=None):
    """What cf_time_steps_coupled needs under CF_HALO_PEER: exports this rank's halo mailbox (`max_fields` fields × `rows` rows,
    ring + 1 by default) and its reduce mailbox, gathers the handles of both over torch.distributed and connects — the slab
    neighbours for the halo rows, every rank for the exact sums (cf_peer_halo_connect, cf_peer_reduce_connect).  A world of one
    (or no process group) connects to nobody: nothing ever waits.  Every rank reaches the gather whatever happened locally, and
    every rank raises when an export failed anywhere, as SlabHaloExchanger agrees on its backend.

    On a tripolar grid the rank this returns as `world − 1` — the one without a north mailbox — passes fold_north = 1 in its
    schedule and every other rank 0: its exchanges fold their own fields as their north side (coupled_fold_plan).  A world of
    one is that last rank."""
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    rows = rows if rows is not None else ctx.grid.ring + 1
    mine, failure = None, None
    try:
        mine = (ctx.peer_halo_export(max_fields=max_fields, max_rows=rows), ctx.peer_reduce_export())
    except Exception as exc:  # noqa: BLE001 — reported below, on every rank
        failure = f"rank {rank}: {exc}"
    gathered = [(mine, failure)]
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, (mine, failure))
    failures = [f for _, f in gathered if f is not None]
    if failures:
        raise RuntimeError("no peer-direct mailboxes: " + "; ".join(failures))
    halo = [h for (h, _r), _ in gathered]
    reduce = [r for (_h, r), _ in gathered]
    ctx.peer_halo_connect(halo[rank - 1] if rank > 0 else None, halo[rank + 1] if rank < world - 1 else None, rank, world)
    ctx.peer_reduce_connect(reduce, rank, world)
    return rank, world


# ---------------------------------------------------------------------------------------------
# The tile world: a px × py partition of the surface (include/coflux.h: cf_peer_tile_*; the reference's
# Partition(2,2), examples/sixth_degree_tripolar_ocean_sea_ice.jl:22).  rank = p + px · q, x fastest.
# ---------------------------------------------------------------------------------------------
def tile_coords(rank, px):
    """(p, q) of `rank`: its column and row of ranks."""
    return rank % px, rank // px


def tile_bounds(nx, ny, rank, px, py):
    """(i0, i1, j0, j1): the columns [i0, i1) and rows [j0, j1) `rank` owns.  Equal tile widths (px divides nx: the fold maps a
    tile onto a whole tile only then); row blocks as slab_bounds cuts them."""
    if nx % px:
        raise ValueError(f"nx = {nx} is no multiple of px = {px}: tiles are equally wide")
    p, q = tile_coords(rank, px)
    nxl = nx // px
    j0, j1 = slab_bounds(ny, q, py)
    return p * nxl, (p + 1) * nxl, j0, j1


def fold_partner(rank, px, py):
    """The rank whose rows fold onto `rank`'s north halo on a tripolar world: (px − 1 − p, py − 1) for a rank of the top row
    (itself when px = 1), None for every other rank."""
    p, q = tile_coords(rank, px)
    return (px - 1 - p) + px * q if q == py - 1 else None


def connect_tiles(ctx, px, py, tripolar, max_fields=4, rows=None, cols=None):
    """What cf_time_steps needs under CF_HALO_PEER on a px × py world: exports this rank's tile mailbox (`max_fields` fields ×
    `rows` rows × `cols` columns; ring + 1 rows and ring + 2 columns by default, which serves the top row of a tripolar world
    too), gathers the handles over torch.distributed and connects (cf_peer_tile_connect).  The process group's rank is the tile
    rank p + px · q.  Every rank reaches the gather whatever happened locally, and every rank raises when an export failed
    anywhere, as connect_coupled_slabs does.  Returns (rank, p, q); the ranks with q = py − 1 of a tripolar world pass
    fold_north = 1 in their schedules, every other rank 0."""
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    if world != px * py:
        raise ValueError(f"a {px} x {py} tile world needs {px * py} ranks, the process group has {world}")
    rows = rows if rows is not None else ctx.grid.ring + 1
    cols = cols if cols is not None else ctx.grid.ring + 2
    mine, failure = None, None
    try:
        mine = ctx.peer_tile_export(max_fields=max_fields, max_rows=rows, max_cols=cols)
    except Exception as exc:  # noqa: BLE001 — reported below, on every rank
        failure = f"rank {rank}: {exc}"
    gathered = [(mine, failure)]
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, (mine, failure))
    failures = [f for _, f in gathered if f is not None]
    if failures:
        raise RuntimeError("no tile mailboxes: " + "; ".join(failures))
    ctx.peer_tile_connect([h for h, _ in gathered], px, py, rank, tripolar)
    return (rank,) + tile_coords(rank, px)


def exchange_tile_halos_reference(tiles, px, py, hx, hy, ring=1, rows=None, tripolar=False, locations=None, signs=None):
    """The tile exchange on NumPy arrays in one process, in place: tiles[rank][f] is field f of `rank`, halo-inclusive
    (ny_q + 2hy, nxl + 2hx).  A plain statement of what cf_halo_exchange_tile_peer leaves — footprint included — written from
    the global picture, not from the kernels:

      x-phase (px > 1): the interior rows of the ring + 1 west halo columns come from the west neighbour's last interior columns,
        those of the east halo columns from the east neighbour's first — ring + 2 east columns on the top row of a tripolar
        world, whose x-face fold reads one column further;
      y-phase: the `rows` south and north halo rows, full width, from the neighbours' boundary rows as the x-phase left them;
        on the top row of a tripolar world the north halo rows, columns −(ring + 1) … nxl + ring only, are the fold of the GLOBAL
        rows: the value at global column g comes from global column Nx − 1 − g (centres, y-faces) or Nx − g (x-faces, |sign| where
        g ≡ 0), read from the partner's array at the image nearest its interior.  With px = 1 the fold is the rank's own, full
        width from the periodic image, and the x-halos stay the caller's."""
    import numpy as np
    rows = ring + 1 if rows is None else rows
    cols = ring + 1
    nfields = len(tiles[0])
    locations = locations or ["center"] * nfields
    signs = signs or [1.0] * nfields
    shape = lambda r: (tiles[r][0].shape[0] - 2 * hy, tiles[r][0].shape[1] - 2 * hx)   # noqa: E731  (ny, nxl)
    nxl = shape(0)[1]
    Nx = px * nxl
    if px > 1:
        incoming = []
        for r in range(px * py):
            p, q = tile_coords(r, px)
            ny = shape(r)[0]
            east_cols = cols + (1 if tripolar and q == py - 1 else 0)
            west, east = (p - 1) % px + px * q, (p + 1) % px + px * q
            for f in range(nfields):
                incoming.append((r, f, slice(hx - cols, hx), tiles[west][f][hy:hy + ny, hx + nxl - cols:hx + nxl].copy()))
                incoming.append((r, f, slice(hx + nxl, hx + nxl + east_cols), tiles[east][f][hy:hy + ny, hx:hx + east_cols].copy()))
        for r, f, where, values in incoming:
            tiles[r][f][hy:hy + shape(r)[0], where] = values
    incoming = []
    for r in range(px * py):
        p, q = tile_coords(r, px)
        ny = shape(r)[0]
        for f in range(nfields):
            if q > 0:
                south = tiles[p + px * (q - 1)][f]
                incoming.append((r, f, slice(hy - rows, hy), slice(None), south[south.shape[0] - hy - rows:south.shape[0] - hy].copy()))
            if q < py - 1:
                incoming.append((r, f, slice(hy + ny, hy + ny + rows), slice(None), tiles[p + px * (q + 1)][f][hy:hy + rows].copy()))
            elif tripolar and px > 1:
                partner = tiles[fold_partner(r, px, py)][f]
                g0_partner = (px - 1 - p) * nxl
                i = np.arange(-cols, nxl + cols)
                g = (p * nxl + i) % Nx                                   # the global periodic image of my column
                block = np.empty((rows, i.size))
                for k in range(1, rows + 1):
                    if locations[f] == "x_face":
                        gs, js, sg = (Nx - g) % Nx, ny - 1 - k, np.where(g == 0, abs(signs[f]), signs[f])
                    elif locations[f] == "y_face":
                        gs, js, sg = Nx - 1 - g, ny - k, signs[f]
                    else:
                        gs, js, sg = Nx - 1 - g, ny - 1 - k, signs[f]
                    local = gs - g0_partner                               # … in the partner's columns, at the image nearest its interior
                    images = np.stack([local - Nx, local, local + Nx])
                    distance = np.maximum(0, np.maximum(-images, images - (nxl - 1)))
                    local = np.take_along_axis(images, np.argmin(distance, axis=0)[None], axis=0)[0]
                    block[k - 1] = sg * partner[hy + js, hx + local]
                incoming.append((r, f, slice(hy + ny, hy + ny + rows), slice(hx - cols, hx + nxl + cols), block))
    for r, f, where_j, where_i, values in incoming:
        tiles[r][f][where_j, where_i] = values
    if tripolar and px == 1:
        from .synthetic import fold_north
        r = px * py - 1
        for f in range(nfields):
            fold_north(tiles[r][f], nxl, shape(r)[0], hx, hy, rows, locations[f], signs[f])
    return tiles


# ---------------------------------------------------------------------------------------------
# Diagnostics on a sharded run: the host's combination of per-rank results into the single domain's (the "Slabs" sentences
# of include/coflux.h).  NumPy only, no device code.  Running means, climatologies and their weights need no combination:
# each rank holds its own rows and columns of the single domain's arrays.
# ---------------------------------------------------------------------------------------------
def _order_key(x):
    """the IEEE total order of the non-NaN doubles as an unsigned integer (include/coflux.h, cf_monitor: "Order")"""
    import struct
    b = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    return b ^ 0xFFFFFFFFFFFFFFFF if b >> 63 else b ^ (1 << 63)


def combine_monitor_records(per_rank):
    """The whole surface's cf_monitor_value records from the ranks' (include/coflux.h, cf_monitor: "Slabs and tiles"), every
    rank having monitored its part with first_cell = j0·Nx + i0 and row_length = Nx.  `per_rank`: arrays of
    abi.MONITOR_VALUE_DTYPE of one shape (a value, a record [n_entries], a series [n, n_entries]); returns that shape.
    minimum / maximum combine in the IEEE total order (−0.0 < +0.0) with the smaller argmin / argmax on ties, −1 and ±Inf where
    no rank has a cell; nan_count / inf_count add; first_nonfinite is the smallest that is not −1; hashes add mod 2⁶⁴."""
    import numpy as np
    from . import abi
    ranks = [np.asarray(r, dtype=abi.MONITOR_VALUE_DTYPE) for r in per_rank]
    if not ranks or any(r.shape != ranks[0].shape for r in ranks):
        raise ValueError("combine_monitor_records: one array of records per rank, all of one shape")
    out = np.zeros(ranks[0].shape, dtype=abi.MONITOR_VALUE_DTYPE)
    flat = out.reshape(-1)
    for at in range(flat.size):
        values = [r.reshape(-1)[at] for r in ranks]
        lo = min(((_order_key(v["minimum"]), int(v["argmin"]), v["minimum"]) for v in values if v["argmin"] >= 0), key=lambda x: x[:2], default=None)
        hi = min(((-_order_key(v["maximum"]), int(v["argmax"]), v["maximum"]) for v in values if v["argmax"] >= 0), key=lambda x: x[:2], default=None)
        V = flat[at]
        V["minimum"], V["argmin"] = (lo[2], lo[1]) if lo else (np.inf, -1)
        V["maximum"], V["argmax"] = (hi[2], hi[1]) if hi else (-np.inf, -1)
        V["nan_count"] = sum(int(v["nan_count"]) for v in values)
        V["inf_count"] = sum(int(v["inf_count"]) for v in values)
        V["first_nonfinite"] = min((int(v["first_nonfinite"]) for v in values if v["first_nonfinite"] >= 0), default=-1)
        V["hash"] = sum(int(v["hash"]) for v in values) % (1 << 64)
    return out


def combine_integral_records(per_rank):
    """The whole surface's integrals from the ranks' (include/coflux.h, cf_integrals: "Slabs"): per record and entry the sum
    over the ranks.  `per_rank`: float64 arrays of one shape; returns that shape.

    Rounding: each entry is math.fsum of the ranks' values — the exact sum of the doubles given, rounded once, so the result
    does not depend on the order of the ranks.  It is NOT the bits of the single domain's record: every rank's value already
    carries the rounding of its own device sum (a fixed order over its own cells), and the single domain adds the same terms in
    another order.  Both lie within γ(n − 1) · Σ|term| of the exact sum of their n terms, γ(n) = n·u / (1 − n·u), u = 2⁻⁵³;
    the combination adds at most one more rounding, u · |result|.  A NaN or an infinity in any rank's entry gives what IEEE
    addition gives (math.fsum raises on Inf − Inf; that entry is NaN here)."""
    import math
    import numpy as np
    ranks = [np.asarray(r, dtype=np.float64) for r in per_rank]
    if not ranks or any(r.shape != ranks[0].shape for r in ranks):
        raise ValueError("combine_integral_records: one array of records per rank, all of one shape")
    out = np.zeros(ranks[0].shape)
    flat = out.reshape(-1)
    for at in range(flat.size):
        terms = [float(r.reshape(-1)[at]) for r in ranks]
        try:
            flat[at] = math.fsum(terms)
        except (ValueError, OverflowError):   # Inf − Inf, or an intermediate overflow: plain IEEE addition
            with np.errstate(all="ignore"):
                flat[at] = np.add.reduce(np.array(terms))
    return out


def restrict_operator(op, nx_global, i0, i1, j0, j1):
    """The operator a rank applies to its own tile (include/coflux.h, cf_regrid: "Slabs"): the same destination rows, of each
    row the entries whose source cell c = j·nx_global + i lies in the columns [i0, i1) and rows [j0, j1), in their order,
    renumbered to the tile's interior (j − j0)·(i1 − i0) + (i − i0).  `op`: (row_ptr, col, weight) or a SurfaceOperator; returns
    (row_ptr int64, col int32, weight float64).  A row with no entry in the tile is an empty row."""
    import numpy as np
    row_ptr, col, weight = op
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col, weight = np.asarray(col, dtype=np.int64), np.asarray(weight, dtype=np.float64)
    j, i = col // nx_global, col % nx_global
    keep = (i >= i0) & (i < i1) & (j >= j0) & (j < j1)
    kept_before = np.concatenate([[0], np.cumsum(keep)])          # kept entries in front of each position
    local = (j - j0) * (i1 - i0) + (i - i0)
    return kept_before[row_ptr].astype(np.int64), local[keep].astype(np.int32), weight[keep].copy()


def combine_regridded(numerators, coverages):
    """The single domain's CF_REGRID_MEAN from the ranks' CF_REGRID_SUM applies of their restricted operators: Σ_ranks N / Σ_ranks D
    per destination row, NaN where the summed coverage is 0 (no wet source cell on any rank).  `numerators`: per rank an array
    [..., n_rows] (one field, or [n_fields, n_rows]); `coverages`: per rank [n_rows].  The sums run over the ranks in the order
    given, one IEEE addition each."""
    import numpy as np
    N = [np.asarray(n, dtype=np.float64) for n in numerators]
    D = [np.asarray(d, dtype=np.float64) for d in coverages]
    if not N or len(N) != len(D) or any(n.shape != N[0].shape for n in N) or any(d.shape != N[0].shape[-1:] for d in D):
        raise ValueError("combine_regridded: per rank one numerator array [..., n_rows] and one coverage [n_rows]")
    num, cov = N[0].copy(), D[0].copy()
    for n, d in zip(N[1:], D[1:]):
        num, cov = num + n, cov + d
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cov == 0, np.nan, num / np.where(cov == 0, 1.0, cov))
