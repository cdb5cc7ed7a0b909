"""Per-scene, per-kernel statistics of the denoiser launches from the database of
`rocprofv3 --kernel-trace --stats -d <dir> -o denoise -- python tools/denoise_timing.py` (profiles/denoise_kernel_stats.csv).

    python tools/denoise_kernel_stats.py <dir>/denoise_results.db > profiles/denoise_kernel_stats.csv
"""
import sqlite3, collections, csv, sys, re
c = sqlite3.connect(sys.argv[1])
rows = c.execute("select name, grid_x, grid_y, duration from kernels order by start").fetchall()
# frame of each dispatch: the per-pixel kernels cover W*H (1D grid = threads), the filter passes (W/16*16, H/16*16) threads
def frame(name, gx, gy):
    if 'k_denoise_pass' in name:
        return {(1920, 1088): '1080p', (3840, 2160): '2160p'}.get((gx, gy), f'{gx}x{gy}')
    n = gx * gy
    for lab, px in (('1080p', 1920 * 1080), ('2160p', 3840 * 2160)):
        if abs(n - px) < 256: return lab
    return f'{gx}x{gy}'
agg = collections.OrderedDict()
seg, last = 0, None                 # tools/denoise_timing.py runs cornell 1080p, cornell 2160p, interior 1080p in turn
scenes = ['cornell', 'cornell', 'interior']
for name, gx, gy, dur in rows:
    short = re.sub(r'\(.*', '', name)
    if not re.search(r'k_feat|k_denoise|k_traverse_paths', short): continue
    f = frame(name, gx, gy)
    if last is not None and f != last: seg += 1
    last = f
    key = (scenes[seg], short, f)
    a = agg.setdefault(key, [0, 0, 1e18, 0])
    a[0] += 1; a[1] += dur; a[2] = min(a[2], dur); a[3] = max(a[3], dur)
w = csv.writer(sys.stdout)
w.writerow(['scene', 'kernel', 'frame', 'calls', 'total_ns', 'average_ns', 'min_ns', 'max_ns'])
for (sc, k, f), (n, t, mn, mx) in agg.items():
    w.writerow([sc, k, f, n, t, round(t / n), mn, mx])
