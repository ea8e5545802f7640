"""Head against parent over the measure.py results in this directory.

For every `kernel_ms` median in <script>_{parent,head}_{1,2}.json (a number, or
under radiance_samples a {variant: {"median": ...}} table) print the four
figures, the largest |head - parent| over the four pairings, and the parent's
own |run 1 - run 2|; then per script the largest of each.

    python profiles/trace_host/summarise.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SCRIPTS = ("ray_queries", "ray_paths", "ray_radiance", "radiance_samples")


def medians(node, path=()):
    if isinstance(node, dict):
        for k, v in node.items():
            if k == "kernel_ms" and isinstance(v, (int, float)):
                yield "/".join(path), float(v)
            elif k == "kernel_ms" and isinstance(v, dict):
                for name, s in v.items():
                    yield "/".join(path + (name,)), float(s["median"])
            else:
                yield from medians(v, path + (k,))


def load(script, side, run):
    with open(os.path.join(HERE, "%s_%s_%d.json" % (script, side, run))) as f:
        return dict(medians(json.load(f)))


for script in SCRIPTS:
    p1, p2, h1, h2 = (load(script, side, run) for side in ("parent", "head") for run in (1, 2))
    worst_hp = worst_pp = (0.0, "")
    for key in p1:
        hp = max(abs(h - p) / p for h in (h1[key], h2[key]) for p in (p1[key], p2[key]))
        pp = abs(p1[key] - p2[key]) / min(p1[key], p2[key])
        print("%-16s %-44s parent %8.4f %8.4f  head %8.4f %8.4f  head-parent %5.2f %%  parent-parent %5.2f %%"
              % (script, key, p1[key], p2[key], h1[key], h2[key], 100 * hp, 100 * pp))
        worst_hp, worst_pp = max(worst_hp, (hp, key)), max(worst_pp, (pp, key))
    print("%-16s largest head-parent %.2f %% (%s); largest parent-parent %.2f %% (%s)\n"
          % (script, 100 * worst_hp[0], worst_hp[1], 100 * worst_pp[0], worst_pp[1]))
