"""Where the GPU stands idle in a traced run: the gaps between consecutive kernels of a rocprofv3 --kernel-trace CSV,
from k_init to the last kernel, next to the cost of k_chain_flush and of the launch sequences that did nothing.

usage: gap_table.py <kernel_trace.csv> <out.json> [out.md]

A gap is the time from the latest end of all earlier kernels to the start of the next one.  Gaps above 10 us are
listed by size class; the gap that follows a k_chain_flush is a host round trip (synchronise, state download, first
launch of the next batch) and is counted apart.  A launch sequence ends at its k_update; one whose k_update returns
at once was stalled, or enqueued after the loop had ended: its cost is the time from the end of the sequence before it
to the end of its k_update.  (At once: under 4.5 us.  A k_update that returns at once still launches its whole grid and
was traced at 2.7 us and more at 32768 taxa; one that works takes 8 us.)"""
import csv
import json
import sys

import numpy as np

from chain_table import short

BIG_NS = 10_000
IDLE_UPDATE_NS = 4500
CLASSES_US = (10, 20, 40, 80, 160, 320, 1000, 10 ** 9)


def main():
    trace, out = sys.argv[1], sys.argv[2]
    rows = []
    with open(trace) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    first = next(i for i, r in enumerate(rows) if r[2] == "k_init")
    rows = rows[first:]
    gaps, after_flush = [], []
    flush_ns, flush_n = 0, 0
    end = rows[0][1]
    for i in range(1, len(rows)):
        s, e, k = rows[i]
        g = s - end
        if g > 0:
            gaps.append(g)
            if rows[i - 1][2] == "k_chain_flush":
                after_flush.append(g)
        if k == "k_chain_flush":
            flush_ns += e - s
            flush_n += 1
        end = max(end, e)
    gaps = np.array(gaps, dtype=np.int64)
    big = gaps[gaps > BIG_NS]
    hist, lo = [], 10
    for hi in CLASSES_US[1:]:
        sel = big[(big > lo * 1000) & (big <= hi * 1000)]
        hist.append({"from_us": lo, "to_us": None if hi == 10 ** 9 else hi, "count": int(sel.size), "sum_ms": round(float(sel.sum()) / 1e6, 3)})
        lo = hi
    # launch sequences that did nothing: every k_update that returned at once, with the time since the sequence before it ended
    idle_n, idle_ns, idle_tail_n, idle_tail_ns = 0, 0, 0, 0
    last_live = max((i for i, r in enumerate(rows) if r[2] == "k_update" and r[1] - r[0] >= IDLE_UPDATE_NS), default=-1)
    seq_end = rows[0][1]
    for i, (s, e, k) in enumerate(rows):
        if k == "k_update":
            if e - s < IDLE_UPDATE_NS:
                if i > last_live:
                    idle_tail_n += 1
                    idle_tail_ns += e - seq_end
                else:
                    idle_n += 1
                    idle_ns += e - seq_end
            seq_end = e
        elif k == "k_chain_flush":
            seq_end = e
    af = np.array(after_flush, dtype=np.int64)
    span = rows[-1][1] - rows[0][0]
    busy = sum(e - s for s, e, _ in rows)
    res = {
        "kernels": len(rows), "span_s": round(span / 1e9, 4), "kernel_busy_s": round(busy / 1e9, 4),
        "gaps_all": {"count": int(gaps.size), "sum_ms": round(float(gaps.sum()) / 1e6, 3), "median_us": round(float(np.median(gaps)) / 1e3, 2) if gaps.size else None},
        "gaps_above_10us": {"count": int(big.size), "sum_ms": round(float(big.sum()) / 1e6, 3), "by_size": hist},
        "gap_after_k_chain_flush": {"count": int(af.size), "sum_ms": round(float(af.sum()) / 1e6, 3),
                                    "median_us": round(float(np.median(af)) / 1e3, 2) if af.size else None,
                                    "p10_us": round(float(np.percentile(af, 10)) / 1e3, 2) if af.size else None,
                                    "p90_us": round(float(np.percentile(af, 90)) / 1e3, 2) if af.size else None,
                                    "max_us": round(float(af.max()) / 1e3, 2) if af.size else None},
        "k_chain_flush": {"launches": flush_n, "sum_ms": round(flush_ns / 1e6, 3)},
        "stalled_sequences": {"count": idle_n, "sum_ms": round(idle_ns / 1e6, 3)},
        "sequences_after_the_last_event": {"count": idle_tail_n, "sum_ms": round(idle_tail_ns / 1e6, 3)},
    }
    json.dump(res, open(out, "w"), indent=1)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write("| item | count | total (ms) |\n|---|---|---|\n")
            f.write(f"| gaps between kernels, all | {res['gaps_all']['count']} | {res['gaps_all']['sum_ms']} |\n")
            f.write(f"| gaps above 10 us | {res['gaps_above_10us']['count']} | {res['gaps_above_10us']['sum_ms']} |\n")
            for h in hist:
                f.write(f"| ... {h['from_us']} to {h['to_us'] if h['to_us'] else 'more'} us | {h['count']} | {h['sum_ms']} |\n")
            a = res["gap_after_k_chain_flush"]
            f.write(f"| gap after k_chain_flush (median {a['median_us']} us, p10 {a['p10_us']}, p90 {a['p90_us']}, max {a['max_us']}) | {a['count']} | {a['sum_ms']} |\n")
            f.write(f"| k_chain_flush | {flush_n} | {res['k_chain_flush']['sum_ms']} |\n")
            f.write(f"| stalled launch sequences | {idle_n} | {res['stalled_sequences']['sum_ms']} |\n")
            f.write(f"| launch sequences after the last event | {idle_tail_n} | {res['sequences_after_the_last_event']['sum_ms']} |\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
