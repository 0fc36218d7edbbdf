"""The tile world on the host (coflux/distributed.py: tile_bounds, tile_coords, fold_partner, exchange_tile_halos_reference;
coflux/synthetic.py: the tile cuts): the partition covers the grid once, the fold's partner map is an involution, and the plain
NumPy exchange — x-phase, y-phase, the partner fold — reproduces the GLOBAL halo-inclusive array, whose x is periodic and whose
fold is coflux.synthetic.fold_north's, on every cell within ring + 1 of every tile's interior, corners included, bit for bit.
Every element names its field, global column and global row (tests/tile_case.py)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tile_case as tc
from coflux import synthetic as syn
from coflux.distributed import exchange_tile_halos_reference, fold_partner, tile_bounds, tile_coords

WORLDS = [(2, 1), (2, 2), (4, 2), (1, 3)]


@pytest.mark.parametrize("px,py", WORLDS + [(4, 1), (1, 1), (6, 1)])
def test_tiles_cover_the_grid_exactly_once_and_partners_pair_up(px, py):
    for nx, ny in ((6 * px, 3 * py), (34 * px, 6 * py + 1)):
        owner = np.zeros((ny, nx), int)
        widths = set()
        for rank in range(px * py):
            assert tile_coords(rank, px) == (rank % px, rank // px)          # x fastest
            i0, i1, j0, j1 = tile_bounds(nx, ny, rank, px, py)
            owner[j0:j1, i0:i1] += 1
            widths.add(i1 - i0)
        assert (owner == 1).all() and widths == {nx // px}
    for rank in range(px * py):
        partner = fold_partner(rank, px, py)
        if rank // px < py - 1:
            assert partner is None
            continue
        assert fold_partner(partner, px, py) == rank and partner // px == py - 1
        assert (partner == rank) == (px == 1)
        # the partner owns the mirror image of this rank's columns
        i0, i1, *_ = tile_bounds(6 * px, 3 * py, rank, px, py)
        m0, m1, *_ = tile_bounds(6 * px, 3 * py, partner, px, py)
        assert (6 * px - i1, 6 * px - i0) == (m0, m1)
    with pytest.raises(ValueError):
        tile_bounds(6 * px + 1, 3 * py, 0, px, py) if px > 1 else tile_bounds(7, 3, 0, 2, 1)


@pytest.mark.parametrize("tripolar", [False, True])
@pytest.mark.parametrize("px,py", WORLDS)
def test_reference_exchange_reproduces_the_global_array_on_the_footprint(px, py, tripolar):
    checked = 0
    for nxl, nyg in tc.shapes(py):
        nxg = px * nxl
        if tripolar and nxg % 2:
            continue                                    # (a tripolar grid has an even number of columns: 3 × 1 tiles are none)
        fields = tc.global_fields(nxg, nyg, len(tc.FIELDS), tripolar)
        tiles = tc.cut_tiles(fields, nxg, nyg, px, py)
        before = [[t.copy() for t in mine] for mine in tiles]
        exchange_tile_halos_reference(tiles, px, py, tc.HX, tc.HY, ring=tc.RING, rows=tc.ROWS, tripolar=tripolar,
                                      locations=[loc for loc, _ in tc.FIELDS], signs=[sg for _, sg in tc.FIELDS])
        for rank in range(px * py):
            i0, i1, j0, j1 = tile_bounds(nxg, nyg, rank, px, py)
            rows, cols = tc.defined_window(rank, px, py, j1 - j0, tripolar)
            for f, g in enumerate(fields):
                want = g[j0:j1 + 2 * tc.HY, i0:i1 + 2 * tc.HX]
                same = tc.same_bits(tiles[rank][f][rows, cols], want[rows, cols])
                assert same.all(), ((px, py), (nxl, nyg), "rank", rank, "field", f, tc.FIELDS[f], "wrong at (row, column) of the window",
                                    np.argwhere(~same)[:6].tolist())
                assert not np.isnan(want[rows, cols]).any()
                # the interior is nobody's to write
                assert tc.same_bits(tiles[rank][f][tc.HY:tc.HY + j1 - j0, tc.HX:tc.HX + nxl],
                                    before[rank][f][tc.HY:tc.HY + j1 - j0, tc.HX:tc.HX + nxl]).all()
                checked += 1
        if tripolar:   # the field of zeros really carries both zeros into folded halos
            top = px * py - 1
            j0, j1 = tile_bounds(nxg, nyg, top, px, py)[2:]
            halo = tiles[top][tc.ZEROS_FIELD][tc.HY + j1 - j0:tc.HY + j1 - j0 + tc.ROWS, tc.HX - tc.COLS:tc.HX + nxl + tc.COLS]
            assert (halo == 0).any() and np.signbit(halo[halo == 0]).any() and (~np.signbit(halo[halo == 0])).any()
    assert checked


def test_tile_cuts_of_the_synthetic_cases_are_the_global_arrays_columns():
    nx, ny, h = 12, 9, 3
    whole = syn.tripolar_case(nx, ny, h, h)
    for rank in range(4):
        i0, i1, j0, j1 = tile_bounds(nx, ny, rank, 2, 2)
        tile = syn.tripolar_tile_case(nx, ny, h, h, i0=i0, i1=i1, j0=j0, j1=j1)
        assert (tile["nx"], tile["ny"]) == (i1 - i0, j1 - j0) and tile["src"].keys() == whole["src"].keys()
        for group in ("ocean", "weights"):
            for k, v in whole[group].items():
                if isinstance(v, np.ndarray):
                    np.testing.assert_array_equal(tile[group][k], v[j0:j1 + 2 * h, i0:i1 + 2 * h], err_msg=f"{group}.{k}")
        flat = syn.latlon_tile_case(nx, ny, h, h, i0=i0, i1=i1, j0=j0, j1=j1, step=1)
        slab = syn.evolved_ocean_state(syn.ocean_state(nx, j1 - j0, h, h, ny_global=ny, j_offset=j0), nx, j1 - j0, h, h, 1, ny_global=ny, j_offset=j0)
        for k in ("T", "S", "u", "v"):
            np.testing.assert_array_equal(flat["ocean"][k], slab[k][:, i0:i1 + 2 * h], err_msg=k)
        assert flat["weights"]["fi"].shape == (i1 - i0 + 2 * h,) and flat["weights"]["fj"].shape == (j1 - j0 + 2 * h,)


def _sanitized_driver(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    compiler = shutil.which("g++") or shutil.which("clang++")
    if compiler is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "tile_geometry_driver")
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(compiler) == "g++" else ["-static-libsan"]
    build = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I",
                            os.path.join(root, "climaocean.jl_amd", "csrc"), os.path.join(root, "tests", "tile_geometry_driver.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find.*(asan|ubsan|clang_rt)|libasan|libubsan|asan_preinit|static-lib", build.stderr):
        pytest.skip("the sanitizer runtime does not link here: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr

    def ask(lines):
        run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
        answers = run.stdout.strip().splitlines()
        assert len(answers) == len(lines)
        return answers
    return ask


def test_the_host_arithmetic_of_the_tile_world_under_the_sanitizers(tmp_path):
    """csrc/coflux_tile_geometry.hpp — the world's refusals, every rank's neighbours, fold partner and the side of their mailboxes
    it writes, the slot sizes and offsets of a mailbox, the tuple comparison — in a stand-alone program built with
    -fsanitize=address,undefined (the runtimes linked statically; nothing is preloaded), against the Python statement of the same
    world.  The program writes the first and last double of both parities of every slot of a heap block of exactly the
    mailbox's size: an offset or a size that is off reports."""
    ask = _sanitized_driver(tmp_path)
    W, E, S, N = range(4)
    questions, want = [], []
    for px in range(0, 10):
        for py in range(0, 6):
            for tripolar in (0, 1):
                for nxl in (3, 4):
                    for rank in range(-1, max(px * py, 0) + 1):
                        questions.append(f"world {px} {py} {rank} {tripolar} {nxl}")
                        if px < 1 or py < 1 or px * py > 8 or not 0 <= rank < px * py or (px > 1 and px % 2) or (tripolar and (px * nxl) % 2):
                            want.append("refused")
                            continue
                        p, q = tile_coords(rank, px)
                        top = q == py - 1
                        partner = fold_partner(rank, px, py) if tripolar and top and px > 1 else None
                        nb = [(p - 1) % px + px * q if px > 1 else -1, (p + 1) % px + px * q if px > 1 else -1, rank - px if q else -1,
                              partner if partner is not None else (-1 if top else rank + px)]
                        sides = [E, W, N, N if partner is not None else S]
                        want.append(" ".join(map(str, [p, q, *nb, *sides, int(top), int(partner is not None)])))
    notes = [(1, 1, 1, 3, 1, 1, 1), (4, 2, 3, 42, 12, 5, 5), (8, 3, 4, 17, 7, 4, 3), (8, 5, 5, 2170, 540, 5, 5)]
    for mf, mr, mc, sj, ny, hx, hy in notes:
        questions.append("note " + " ".join(map(str, (mf, mr, mc, sj, ny, hx, hy))))
        xs, ys = mf * mc * ny, mf * mr * sj
        data = 9 * 64
        want.append(" ".join(map(str, [xs, ys, data + 8 * 4 * (xs + ys), data, data + 16 * xs, data + 32 * xs, data + 32 * xs + 16 * ys])))
    mine = (4, 2, 3, 42, 12, 5, 4)
    for side in range(4):
        for k in range(7):
            theirs = list(mine)
            theirs[k] += 1
            questions.append(f"agree {side} " + " ".join(map(str, mine)) + " " + " ".join(map(str, theirs)))
            # what the mailboxes take always; W and E: ny and hy; S, N and the partner: nx + 2hx and hx
            matters = k < 3 or (k in (4, 6) if side < S else k in (3, 5))
            want.append(f"{0 if matters else 1} (max_fields, max_rows, max_cols, nx + 2hx, ny, hx, hy) = ({', '.join(map(str, theirs))})")
    for ring in (0, 1):
        for fold in (0, 1):
            questions.append(f"columns {ring} {fold}")
            want.append(f"{ring + 1} {ring + 1 + fold}")
    got = ask(questions)
    wrong = [(q, g, w) for q, g, w in zip(questions, got, want) if g != w]
    assert not wrong, wrong[:10]
