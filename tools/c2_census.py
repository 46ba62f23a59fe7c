#!/usr/bin/env python3
"""When do the tiles of the C2 exchange kernel finish?  (profiling aid; the env knobs are debug-only)

usage: python tools/c2_census.py [launches]          (TUNE_SIZE: the image's side, 16384)
Runs the driver's image through the census build of reduce_fused_u8x4_mfma_x ($VIPS_HIP_FUSED_DEBUG=1024: thread 0
of every block stamps the chip-wide 100 MHz clock at kernel entry, after the prologue, when the row loop is done and
after the block's last store; $VIPS_HIP_FUSED_CENSUS: the launcher appends the slots to a file) after a warm-up, and
prints, in microseconds after the launch's earliest entry, the median and the spread of "loop done" and "end done"
for the interior tiles, the left and right columns, the top and bottom rows and every XCD, and how much later than
the median tile the last tile of each launch finishes.
"""
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TICK_US = 0.01  # s_memrealtime: 100 MHz


def parse(path):
    """-> launches: lists of (tile, bx, by, block, xcc, entry, prologue, loop_done, end_done), and (tiles_x, tiles_y) each."""
    launches, shapes = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("#"):
                words = line.split()
                shapes.append((int(words[2]), int(words[4])))
                launches.append([])
            elif line.strip():
                launches[-1].append(tuple(int(v) for v in line.split()))
    return launches, shapes


def spread(values):
    v = sorted(values)
    pick = lambda q: v[min(len(v) - 1, int(q * len(v)))]
    return statistics.median(v) * TICK_US, pick(0.05) * TICK_US, pick(0.95) * TICK_US, v[0] * TICK_US, v[-1] * TICK_US


def table(launches, shapes):
    groups = {}

    def add(name, row):
        groups.setdefault(name, []).append(row)

    for rows, (tx, ty) in zip(launches, shapes):
        for row in rows:
            _, bx, by, _, xcc = row[:5]
            col_edge = bx == 0 or bx == tx - 1
            row_edge = by == 0 or by == ty - 1
            if col_edge:
                add("left / right column", row)
            if row_edge:
                add("top / bottom row", row)
            if not col_edge and not row_edge:
                add("interior", row)
            add("XCD %d" % xcc, row)
    out = ["%-20s %6s | %-44s | %-44s" % ("tiles", "n", "loop done: med   p5   p95   min   max (us)", "end done: med   p5   p95   min   max (us)")]
    for name in ["interior", "left / right column", "top / bottom row"] + sorted(g for g in groups if g.startswith("XCD")):
        rows = groups.get(name, [])
        if not rows:
            continue
        loop = spread([r[7] for r in rows])
        end = spread([r[8] for r in rows])
        out.append("%-20s %6d | %10.2f %6.2f %6.2f %6.2f %6.2f %6s | %10.2f %6.2f %6.2f %6.2f %6.2f"
                   % ((name, len(rows)) + loop + ("",) + end))
    out.append("")
    out.append("per launch: entry of the last tile to start, median / last loop done, median / last end done, last - median (us), the last tile")
    for rows in launches:
        entry = max(r[5] for r in rows) * TICK_US
        loop = [r[7] for r in rows]
        end = [r[8] for r in rows]
        last = max(rows, key=lambda r: r[8])
        out.append("  entry %6.2f | loop %7.2f %7.2f | end %7.2f %7.2f | +%5.2f | tile (%d, %d) XCD %d"
                   % (entry, statistics.median(loop) * TICK_US, max(loop) * TICK_US, statistics.median(end) * TICK_US,
                      max(end) * TICK_US, (max(end) - statistics.median(end)) * TICK_US, last[1], last[2], last[4]))
    return "\n".join(out)


def main():
    import torch

    import libvips_amd
    from bench import lcg_image_device
    from libvips_amd import Image

    n_launches = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    device = torch.device("cuda", 0)
    libvips_amd.init(0)
    n = int(os.environ.get("TUNE_SIZE", "16384"))
    src = lcg_image_device(torch, n, n, 4, 12345, device)
    torch.cuda.synchronize()
    im = Image.new_from_tensor(src)
    extra = int(os.environ.get("VIPS_HIP_FUSED_DEBUG", "0"))
    os.environ["VIPS_HIP_FUSED_DEBUG"] = str(extra | 1024)
    for _ in range(20):
        im.reduce(8.0, 8.0, kernel="lanczos3")
    torch.cuda.synchronize()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "census.txt")
        os.environ["VIPS_HIP_FUSED_CENSUS"] = path
        for _ in range(n_launches):
            # (NOT back to back as the benchmark's steps are: the launcher waits for each census launch to copy its
            # slots back, so every launch starts on an idle part)
            im.reduce(8.0, 8.0, kernel="lanczos3")
        torch.cuda.synchronize()
        del os.environ["VIPS_HIP_FUSED_CENSUS"]
        launches, shapes = parse(path)
    if not launches:
        sys.exit("no census lines: is the library's census build reached ($VIPS_HIP_FUSED_DEBUG=1024)?")
    print("%d launches of %d x %d tiles (%d x %d RGBA uchar)" % (len(launches), shapes[0][0], shapes[0][1], n, n))
    print(table(launches, shapes))


if __name__ == "__main__":
    main()
