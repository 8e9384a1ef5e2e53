#!/usr/bin/env python3
"""Where the main stream of the prover runs no kernel: gaps in a rocprofv3 --kernel-trace.

    python3 tools/stream_gaps.py <kernel_trace.csv> [--compact OUT.csv]

Reads the start and end timestamps, queue ids, stream ids and names of the trace (nothing else has
to be traced) and prints
  * the stream and the hardware queue of every kernel family (quotient and accumulate launches:
    main; solve: stream2; Horner, assembly, multiples of delta: stream3; msm_reduce and, with a
    deferred tail, comb_common_sums: the MSM tail): two stream ids with one queue id are two streams
    that the runtime put on one hardware queue.  A trace without stream ids (all zero) is read by
    queue id alone;
  * per step, for the G1 stage -- from the last NTT kernel to the last G1 accumulate launch -- the
    sum of the gaps between consecutive kernels of the main stream and the five largest gaps with the
    kernel that follows each (#n: its n-th launch of the stage; the MSMs run in the order A, B1, K,
    Z, so comb_split_kernel #3 opens K);
  * per step, how long after each G1 accumulate launch its first msm_reduce pass started.
The main stream is the one the NTT kernels run on.  --compact writes the trace with short names
(queue, stream, start and end in ns from the first kernel, name), small enough to keep beside the
output.
"""
import argparse
import csv
import re
import sys


def short(name):
    name = name.replace("void ", "").replace("zk::", "")
    name = name.replace("Fp<FqParams>", "Fq").replace("Fp<FrParams>", "Fr")
    m = re.match(r"([A-Za-z_0-9:]+)(<.*?>)?\(", name)
    if not m:
        return name.split("(")[0]
    targs = m.group(2) or ""
    if len(targs) > 24:
        targs = targs[:21] + "...>"
    return m.group(1) + targs


def family(s):
    if s.startswith("ntt_") or s.startswith("pointwise") or s.startswith("quot"):
        return "quotient"
    for key, fam in (("msm_accumulate_comb", "accumulate"), ("msm_accumulate_shared", "accumulate"),
                     ("msm_accumulate<", "delta multiples"), ("msm_reduce", "msm_reduce"),
                     ("comb_common_sums", "comb_common_sums"), ("comb_digits", "digits / split"),
                     ("comb_split", "digits / split"), ("comb_scalars", "digits / split"),
                     ("rows_vary", "digits / split"), ("msm_horner", "horner / assembly"),
                     ("comb_fold8", "horner / assembly"), ("assemble", "horner / assembly"),
                     ("solve_", "solve")):
        if key in s:
            return fam
    return None


def load(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                         (int(r["Queue_Id"]), int(r.get("Stream_Id") or 0)),
                         short(r["Kernel_Name"])))
    rows.sort()
    if any(q[1] for _, _, q, _ in rows):
        return rows, True
    return [(s, e, (q[0], q[0]), n) for s, e, q, n in rows], False   # the queue stands for the stream


def is_g1_acc(s):
    return s.startswith("msm_accumulate_comb<Fq,") or s.startswith("msm_accumulate_shared<Fq>")


def is_g2_acc(s):
    return s.startswith("msm_accumulate_comb<Fq2") or s.startswith("msm_accumulate_shared<Fq2")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("trace")
    ap.add_argument("--compact", metavar="OUT.csv")
    args = ap.parse_args()
    # rows: (start, end, (queue, stream), name), told apart by stream where the trace has stream ids
    rows, by_stream = load(args.trace)
    if not rows:
        sys.exit("stream_gaps: empty trace")
    t0 = rows[0][0]
    if args.compact:
        with open(args.compact, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["queue", "stream", "start_ns", "end_ns", "kernel"])
            for s, e, q, n in rows:
                w.writerow([q[0], q[1], s - t0, e - t0, n])

    fams = {}
    for s, e, q, n in rows:
        fam = family(n)
        if fam:
            fams.setdefault(fam, {}).setdefault(q, 0)
            fams[fam][q] += 1
    what = "stream s on queue q" if by_stream else "queue q"
    print(f"where every kernel family ran ({what}: launches)")
    for fam in sorted(fams):
        print(f"  {fam:18s} " + ", ".join(
            (f"s{q[1]} on q{q[0]}" if by_stream else f"q{q[0]}") + f": {c}"
            for q, c in sorted(fams[fam].items())))
    ntt_q = {}
    for s, e, q, n in rows:
        if n.startswith("ntt_"):
            ntt_q[q] = ntt_q.get(q, 0) + 1
    if not ntt_q:
        sys.exit("stream_gaps: no NTT kernel in the trace")
    mq = max(ntt_q, key=ntt_q.get)
    print(f"main stream: " + (f"s{mq[1]} on q{mq[0]}" if by_stream else f"q{mq[0]}"))
    main_rows = [r for r in rows if r[2] == mq]

    # steps: [last NTT kernel of a quotient .. last G1 accumulate launch before the G2 one]
    steps = []
    i = 0
    while i < len(main_rows):
        if main_rows[i][3].startswith("ntt_") and i + 1 < len(main_rows) and \
                not main_rows[i + 1][3].startswith("ntt_"):
            j, last_acc = i + 1, None
            while j < len(main_rows) and not main_rows[j][3].startswith("ntt_") and \
                    not is_g2_acc(main_rows[j][3]):
                if is_g1_acc(main_rows[j][3]):
                    last_acc = j
                j += 1
            if last_acc is not None:
                steps.append((i, last_acc))
            i = j
        else:
            i += 1
    if not steps:
        sys.exit("stream_gaps: no G1 stage found on the main queue")

    reduces = [r for r in rows if r[3].startswith("msm_reduce")]
    total = 0.0
    print("step  G1 stage ms  kernels ms  idle ms   five largest gaps: ms before <kernel>")
    for k, (a, b) in enumerate(steps):
        busy_end = main_rows[a][1]
        gaps, kern, seen = [], 0.0, {}
        for r in main_rows[a + 1:b + 1]:
            seen[r[3]] = seen.get(r[3], 0) + 1     # "#3": the third launch of this kernel in the stage
            if r[0] > busy_end:
                gaps.append((r[0] - busy_end, f"{r[3]} #{seen[r[3]]}"))
            kern += r[1] - r[0]
            busy_end = max(busy_end, r[1])
        idle = sum(g for g, _ in gaps)
        total += idle
        top = sorted(gaps, reverse=True)[:5]
        print(f"{k:4d}  {(main_rows[b][1] - main_rows[a][1]) / 1e6:11.3f}  {kern / 1e6:10.3f}  "
              f"{idle / 1e6:7.3f}   " + "; ".join(f"{g / 1e6:.3f} {n}" for g, n in top))
    print(f"mean idle ms per step over {len(steps)} steps: {total / len(steps) / 1e6:.3f}")

    print("step  ms from the end of each G1 accumulate launch to the start of its first msm_reduce")
    for k, (a, b) in enumerate(steps):
        out = []
        for r in main_rows[a + 1:b + 1]:
            if is_g1_acc(r[3]):
                nxt = [x for x in reduces if x[0] >= r[1]]
                out.append(f"{(nxt[0][0] - r[1]) / 1e6:.3f}" if nxt else "-")
        print(f"{k:4d}  " + "  ".join(out))


if __name__ == "__main__":
    main()
