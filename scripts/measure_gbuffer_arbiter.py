"""Measure what tests/test_gbuffer_arbiter.py asserts and write profiles/gbuffer_arbiter.md: per case the depth and position
differences of the G-buffer specification against the float64 arbiter, per class the self-consistent maximum of the normal's angle
(the smallest m, at least the largest angle conditioning does not explain, with no pixel in (m, 2m] and the 3 % cap on exclusions
holding in every case of the class at the bound 2m), and the excluded share per case at that bound.  CPU only.
    python scripts/measure_gbuffer_arbiter.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gbuffer_arbiter as T  # noqa: E402


def class_maximum(ms, gate=None):
    disc = np.concatenate([m["disc"][m["both"]] for m in ms])
    sens = np.concatenate([m["sens"][m["both"]] for m in ms])
    unexplained = float(disc[sens < disc].max()) if (sens < disc).any() else 0.0
    for cand in sorted(set([unexplained] + [float(v) for v in disc[disc >= unexplained]])):
        bound = 2 * cand if gate is None else min(2 * cand, gate)
        if ((disc > cand) & (disc <= bound)).any() or cand == 0.0:
            continue
        if all(T.excluded(m, bound)[2] <= T.CAP for m in ms):
            return cand, unexplained
    raise SystemExit("no self-consistent maximum keeps the cap")


def main():
    per_class = {}
    measured = [(name, cls, T.measure(build, s)) for name, build, s, cls in T.CASES]
    for _, cls, m in measured:
        per_class.setdefault(cls, []).append(m)
    maxima = {cls: class_maximum(ms, T.GATE if cls == "primitives" else None) for cls, ms in per_class.items()}
    rows = []
    for name, cls, m in measured:
        bound = 2 * maxima[cls][0] if cls != "primitives" else min(2 * maxima[cls][0], T.GATE)
        excused, mask, share = T.excluded(m, bound)
        both, kept = m["both"], m["both"] & ~excused
        literal = (m["hit"] & ~(both & (m["sens"] < m["disc"]))).sum() / m["hit"].sum()
        rows.append(f"| {name} | {cls} | {m['scene'][2]} | {m['hit'].sum()} | {(m['hit'] & ~m['clear']).sum()} | {(m['hit'] & m['overshoot']).sum()} | "
                    f"{m['ddepth'][both].max():.2e} | {m['ddepth'][both].max() - T.SURFACE_DIST:+.3e} | {m['dpos'][both].max():.2e} | "
                    f"{m['disc'][kept].max():.2e} | {excused.sum()} | {100 * share:.2f} % | {100 * literal:.0f} % |")
        print(rows[-1], flush=True)
    out = os.path.join(ROOT, "profiles", "gbuffer_arbiter.md")
    head = open(out).read().split("<!-- measured -->")[0] if os.path.exists(out) else ""
    with open(out, "w") as f:
        f.write(head + "<!-- measured -->\n\n| class | measured maximum (rad) | largest angle conditioning does not explain | asserted bound |\n|---|---|---|---|\n")
        for cls, (mx, un) in maxima.items():
            f.write(f"| {cls} | {mx:.3e} | {un:.3e} | {min(2 * mx, T.GATE) if cls == 'primitives' else 2 * mx:.3e} |\n")
        f.write("\n| case | class | objects | hit pixels | not clear | of them unstable | max \\|Δdepth\\| | − SURFACE_DIST | max \\|Δposition\\| | "
                "max angle, not excused (rad) | excused | excluded share | share under the literal rule |\n" + "|---" * 13 + "|\n" + "\n".join(rows) + "\n")
    print({k: f"{v[0]:.3e}" for k, v in maxima.items()})


if __name__ == "__main__":
    main()
