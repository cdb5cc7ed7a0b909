"""Per-launch PMC counters of two committed profile sets, kernel by kernel:
    python tools/compare_pmc.py r07 r08 [workload ...]        (default: every workload both sets have)
Prints, per workload, each kernel's relative change of SQ_INSTS_VALU and TCP_TOTAL_CACHE_ACCESSES_sum and the largest |change|,
and names the kernels found in one set only.  `RENAMED` maps kernel names of the older set to the newer one."""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "TCP_TOTAL_CACHE_ACCESSES_sum")
# r08: the accumulate kernels became templates on MOMENTS; the render runs the <false> instantiations
# r11: the camera-ray generator and the resolve kernel gained a MAPPED parameter (adaptive sampling); the render runs <false>
# r14: the accumulate kernels gained a BUCKETS parameter (robust picture); the render runs <false,false>
RENAMED = {"k_finalize_accumulate": "k_finalize_accumulate<false>", "k_accumulate": "k_accumulate<false>",
           "k_finalize_accumulate<false>": "k_finalize_accumulate<false,false>", "k_accumulate<false>": "k_accumulate<false,false>",
           "k_gen_rays": "k_gen_rays<false>", "k_gen_camera_rays": "k_gen_camera_rays<false>",
           **{f"k_connect_resolve<{a}>": f"k_connect_resolve<{a},false>"
              for a in ("3,true,false", "2,false,false", "2,true,true", "2,false,true")},
           # r19: the resolve kernel gained a STRAT parameter (strategy mask); the render runs <..., false>
           **{f"k_connect_resolve<{a},{m}>": f"k_connect_resolve<{a},{m},false>"
              for a in ("3,true,false", "2,false,false", "2,true,true", "2,false,true") for m in ("false", "true")},
           # r20: the resolve kernel gained a LAYERS parameter (layer accumulators); the render runs <..., false>
           **{f"k_connect_resolve<{a},{m},{s}>": f"k_connect_resolve<{a},{m},{s},false>"
              for a in ("3,true,false", "2,false,false", "2,true,true", "2,false,true") for m in ("false", "true") for s in ("false", "true")}}


def kernels(tag, workload):
    return json.load(open(os.path.join(ROOT, "profiles", f"{tag}_pmc_{workload}.json")))["kernels"]


def main():
    old, new = sys.argv[1], sys.argv[2]
    names = sys.argv[3:] or sorted(os.path.basename(p)[len(f"{new}_pmc_"):-5]
                                   for p in glob.glob(os.path.join(ROOT, "profiles", f"{new}_pmc_*.json"))
                                   if os.path.exists(p.replace(f"{new}_pmc_", f"{old}_pmc_")))
    for w in names:
        a = {RENAMED.get(k, k): v for k, v in kernels(old, w).items()}
        b = kernels(new, w)
        worst = dict.fromkeys(COUNTERS, 0.0)
        rows = []
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                rows.append(f"  {k}: only in {old if k in a else new}")
                continue
            d = {c: 100.0 * (b[k][c] - a[k][c]) / a[k][c] for c in COUNTERS if a[k].get(c) and c in b[k]}
            for c, v in d.items():
                worst[c] = max(worst[c], abs(v))
            rows.append(f"  {k}: " + "  ".join(f"{c} {v:+.3f} %" for c, v in d.items()))
        print(f"{w}: {len(a)} / {len(b)} kernels; largest |change| " + ", ".join(f"{c} {v:.3f} %" for c, v in worst.items()))
        print("\n".join(rows))


if __name__ == "__main__":
    main()
