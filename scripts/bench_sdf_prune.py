#!/usr/bin/env python3
"""rm_sdf_blocks_select_pruned measured against rm_sdf_blocks_select.  One process, one GPU, the routes of a table interleaved round
by round, outputs compared before anything is timed.

  A  the selection alone at the C ABI, exact capacities: S = rm_sdf_blocks_select, P(1, inf), P(1, 1) and P(4, inf) (the Python
     layer's defaults) = rm_sdf_blocks_select_pruned with (lipschitzOut, lipschitzIn); ms, candidates, listed blocks and blocks
     LOST against S's list
  B  the whole mesh through the Python layer: scene_mesh_sparse against scene_mesh_pruned (defaults), meshes compared word for word
  C  a ladder of lipschitzOut at --ladder points per axis: lost blocks, candidates, ms
  D  the blocks lost over the same ladder at every measured size, not timed

Scenes: the headline Mandelbulb (12 iterations, iso 0.001) and c5's sponge (unit_mengersponge.json, 5 levels, iso 0.001), each over
scene_mesh_sparse's lattice of its mesh_bounds.  HIP events around each call, a warm-up round, then --rounds interleaved rounds;
median [min – max].

  python scripts/bench_sdf_prune.py [--bulb 513,1025,2049,4097] [--sponge 513,1025,2049] [--ladder 1025] [--rounds 5] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
INF = float("inf")
LADDER = (0.25, 0.5, 1.0, 2.0, 4.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bulb", default="513,1025,2049,4097")
    ap.add_argument("--sponge", default="513,1025,2049")
    ap.add_argument("--ladder", type=int, default=1025)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import torch
    from raymarcher_amd import Renderer, Scene, abi, lib, scenes

    r = Renderer(0)
    dev = r.device
    L = lib()
    iso = 0.001

    def timed(routes, rounds):
        for fn in routes.values():  # the warm-up round
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        return times

    def fmt(v):
        return f"{statistics.median(v):.3f} [{min(v):.3f} – {max(v):.3f}]"

    def vec(v):
        return (C.c_float * 3)(*[float(x) for x in v])

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

    def table(name):
        if name == "bulb":
            return scenes.mandelbulb(64, 36), abi.default_settings(fractalIters=12), "the headline Mandelbulb, 12 iterations"
        t = Scene(path=os.path.join(SCENES, "simple", "unit_mengersponge.json")).tables(64, 36)
        return t, abi.default_settings(mengerLevels=5), "c5's sponge: unit_mengersponge.json, 5 levels"

    class Selection:
        """The two entries on scene_mesh_sparse's lattice of `points` points per axis, at the C ABI."""

        def __init__(self, t, s, points):
            origin, step, dims = r._scene_lattice(t, points, None)
            self.t, self.s, self.o3, self.s3 = t, s, vec(origin), vec((step,) * 3)
            self.blocks = [(d - 1 + 7) // 8 for d in dims]
            self.count = torch.zeros(2, dtype=torch.int32, device=dev)

        def call(self, constants, capacity, out=None):
            t, mx, my, mz = self.t, *self.blocks
            head = (t.objects, t.num_objects, C.byref(t.globals_), C.byref(self.s), self.o3, self.s3, mx, my, mz, iso)
            fn = L.rm_sdf_blocks_select if constants is None else L.rm_sdf_blocks_select_pruned
            st = fn(*head, *(constants or ()), capacity, ptr(out), ptr(self.count), r._stream())
            assert st == abi.RM_OK, L.rm_last_error().decode()

        def listed(self, constants):
            """(the list, the candidates) through a counting call and one with the exact capacity."""
            self.call(constants, 0)
            n = int(self.count[0].item()) & 0xFFFFFFFF
            out = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
            self.call(constants, n, out)
            again, cand = (int(x) & 0xFFFFFFFF for x in self.count.tolist())
            assert again == n
            return out, (cand if constants is not None else None)

        def linear(self, rows):
            return (rows[:, 2].long() * self.blocks[1] + rows[:, 1]) * self.blocks[0] + rows[:, 0]

    def compare(sel, every, constants):
        """The pruned list against the exhaustive one: a sub-sequence of it → (rows, candidates, lost blocks)."""
        rows, cand = sel.listed(constants)
        a, b = sel.linear(rows), sel.linear(every)
        assert bool((a[1:] > a[:-1]).all()) and bool(torch.isin(a, b).all()) and bool((rows[:, 3] == 0).all()), "not a sub-sequence"
        assert len(rows) < len(every) or torch.equal(rows, every)
        return rows, cand, len(every) - len(rows)

    emit("# rm_sdf_blocks_select_pruned against rm_sdf_blocks_select")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; one process; HIP events around each call, a warm-up round, then {args.rounds} interleaved "
         "rounds; ms per call, median [min – max] over the rounds; iso 0.001; scene_mesh_sparse's lattice over the table's mesh_bounds. "
         "Every pruned list was compared with the exhaustive list of the same lattice before anything was timed: a sub-sequence of it, "
         "equal in every word where no block is lost.")
    lost_at_one = []
    for name, sizes in (("bulb", args.bulb), ("sponge", args.sponge)):
        if not sizes:  # --sponge "": the scene is left out
            continue
        t, s, title = table(name)
        emit()
        emit(f"## {title}")
        emit()
        emit("### A. The selection alone (S = rm_sdf_blocks_select; P(out, in) = rm_sdf_blocks_select_pruned)")
        emit()
        emit("| points per axis | blocks | route | ms per call | candidates | listed blocks | lost | S / P |")
        emit("|---|---|---|---|---|---|---|---|")
        for points in [int(x) for x in sizes.split(",") if x]:
            torch.cuda.empty_cache()
            L.rm_release_workspaces(None)
            sel = Selection(t, s, points)
            total = sel.blocks[0] * sel.blocks[1] * sel.blocks[2]
            every, _ = sel.listed(None)
            variants = {"S": (None, every, None, 0)}
            for constants in ((1.0, INF), (1.0, 1.0), (4.0, INF)):  # the last: the Python layer's defaults
                rows, cand, lost = compare(sel, every, constants)
                variants[f"P({constants[0]:g}, {constants[1]:g})"] = (constants, rows, cand, lost)
                if lost:
                    lost_at_one.append(f"{name} {points}: P({constants[0]:g}, {constants[1]:g}) lost {lost}")
            outs = {k: torch.empty_like(v[1]) for k, v in variants.items()}
            routes = {k: (lambda k=k, v=v: sel.call(v[0], len(v[1]), outs[k])) for k, v in variants.items()}
            times = timed(routes, args.rounds)
            for k, v in variants.items():
                assert torch.equal(outs[k], v[1]), f"{name} {points} {k}: the timed call's list differs"
            base = statistics.median(times["S"])
            for k, (constants, rows, cand, lost) in variants.items():
                emit(f"| {points} | {total} | {k} | {fmt(times[k])} | {cand if cand is not None else total} | {len(rows)} | {lost} | "
                     f"{base / statistics.median(times[k]):.2f} |")
            del every, variants, outs, routes
            flush()
        emit()
        emit("### B. The whole mesh through the Python layer (selection with its capacity protocol, rm_sdf_grid_blocks, rm_sdf_mesh_blocks)")
        emit()
        emit("| points per axis | scene_mesh_sparse ms | scene_mesh_pruned ms | sparse / pruned | vertices | quads | equal in every word |")
        emit("|---|---|---|---|---|---|---|")
        for points in [int(x) for x in sizes.split(",") if x]:
            torch.cuda.empty_cache()
            L.rm_release_workspaces(None)
            a = r.scene_mesh_sparse(t, s, points, iso)
            try:
                b = r.scene_mesh_pruned(t, s, points, iso)
            except RuntimeError as e:  # a lost block cuts the mesh open: recorded, not hidden
                emit(f"| {points} | | scene_mesh_pruned raises: {e} | | {len(a[0])} | {len(a[1])} | NO |")
                flush()
                continue
            same = all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
            nv, nq = len(a[0]), len(a[1])
            del a, b
            times = timed({"sparse": lambda: r.scene_mesh_sparse(t, s, points, iso), "pruned": lambda: r.scene_mesh_pruned(t, s, points, iso)},
                          min(args.rounds, 3) if points > 2049 else args.rounds)
            ratio = statistics.median(times["sparse"]) / statistics.median(times["pruned"])
            emit(f"| {points} | {fmt(times['sparse'])} | {fmt(times['pruned'])} | {ratio:.2f} | {nv} | {nq} | {'yes' if same else 'NO'} |")
            flush()
        emit()
        emit(f"### C. The ladder of lipschitzOut at {args.ladder} points per axis (lipschitzIn = +inf)")
        emit()
        emit("| lipschitzOut | ms per call | candidates | listed blocks | lost |")
        emit("|---|---|---|---|---|")
        torch.cuda.empty_cache()
        L.rm_release_workspaces(None)
        sel = Selection(t, s, args.ladder)
        every, _ = sel.listed(None)
        ladder = {}
        for l_out in LADDER:
            rows, cand, lost = compare(sel, every, (l_out, INF))
            ladder[l_out] = (rows, cand, lost, torch.empty_like(rows))
        times = timed({k: (lambda k=k, v=v: sel.call((k, INF), len(v[0]), v[3])) for k, v in ladder.items()}, args.rounds)
        for l_out, (rows, cand, lost, _out) in ladder.items():
            emit(f"| {l_out:g} | {fmt(times[l_out])} | {cand} | {len(rows)} | {lost} |")
        del every, ladder
        emit()
        emit("### D. Blocks lost over the ladder at every measured size (lipschitzIn = +inf; not timed)")
        emit()
        emit("| points per axis | active blocks | " + " | ".join(f"lost at {v:g}" for v in LADDER) + " |")
        emit("|---|---|" + "---|" * len(LADDER))
        for points in [int(x) for x in sizes.split(",") if x]:
            torch.cuda.empty_cache()
            L.rm_release_workspaces(None)
            sel = Selection(t, s, points)
            every, _ = sel.listed(None)
            emit(f"| {points} | {len(every)} | " + " | ".join(str(compare(sel, every, (v, INF))[2]) for v in LADDER) + " |")
            del every
            flush()
    emit()
    emit("Blocks lost in the tables A: " +
         ("; ".join(lost_at_one) if lost_at_one else "none, on either scene at any measured size."))
    flush()


if __name__ == "__main__":
    main()
