"""Every launch of one kernel family in the last training step of a rocpd kernel trace, with what ran beside it on the other streams:
python scripts/rocpd_beside.py <trace.db> <substring of the kernel name> [<substring that must NOT occur>]
One line per launch: start, duration, then the overlapping kernels of other streams as name:overlap in us."""
import sqlite3
import sys

from rocpd_timeline import short


def main(path, want, unwanted=None):
    db = sqlite3.connect(path)
    rows = db.execute("select name, stream_id, start, end from kernels order by start").fetchall()
    adam = [i for i, r in enumerate(rows) if 'clamp_adam' in r[0]]   # step boundary, as in rocpd_timeline.py
    step = rows[adam[-2] + 1:adam[-1] + 1]
    t0 = step[0][2]
    mine = [r for r in step if want in r[0] and not (unwanted and unwanted in r[0])]
    durs = [(r[3] - r[2]) / 1e3 for r in mine]
    print("%d launches of '%s': min / avg / max %.1f / %.1f / %.1f us, total %.3f ms" %
          (len(mine), want, min(durs), sum(durs) / len(durs), max(durs), sum(durs) / 1e3))
    for r in mine:
        beside = {}
        for o in step:
            if o[1] == r[1] or o[3] <= r[2] or o[2] >= r[3]:
                continue
            beside[short(o[0])[:36]] = beside.get(short(o[0])[:36], 0.0) + (min(o[3], r[3]) - max(o[2], r[2])) / 1e3
        print("  %8.3f ms  %7.1f us  %s" % ((r[2] - t0) / 1e6, (r[3] - r[2]) / 1e3,
                                          ", ".join("%s:%.0f" % kv for kv in sorted(beside.items(), key=lambda kv: -kv[1])[:4]) or "(alone)"))


if __name__ == '__main__':
    main(*sys.argv[1:4])
