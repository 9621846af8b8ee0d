#!/usr/bin/env python3
"""Summarise a rocprofv3 --kernel-trace --memory-copy-trace run of the PIPELINED bench (default: 4 batches in
flight on 4 streams): per stream the sequence k_pack .. k_out_pack, D2H; what the copy engine and the CUs
were doing; how long a stream sits idle between the end of its copy and its next k_pack.  For the paired pump
also each of its streams by itself ("pump_streams": the queue id the trace gives it, what it carries, its busy
time per step) and how often the paired launch started late because the k_pack it waits for had not ended.
usage: timeline_summary.py <trace dir> <out.json>"""
import collections
import csv
import glob
import json
import sys

root, out_path = sys.argv[1], sys.argv[2]


def rows(pattern):
    for path in sorted(glob.glob(root + "/**/" + pattern, recursive=True)):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                yield r


def col(r, *names):
    for n in names:
        if n in r and r[n] != "":
            return r[n]
    return None


kern = []
queue_of = collections.defaultdict(set)                # stream -> the queue ids its rows carry
for r in rows("*kernel_trace.csv"):
    name = (col(r, "Kernel_Name") or "").split("(")[0].replace("void ", "").replace("kmd::", "")
    short = name.split("<")[0]
    kern.append((int(col(r, "Start_Timestamp")), int(col(r, "End_Timestamp")), short,
                 col(r, "Stream_Id", "Queue_Id") or "?"))
    queue_of[kern[-1][3]].add(col(r, "Queue_Id") or "?")
copies = []
for r in rows("*memory_copy_trace.csv"):
    copies.append((int(col(r, "Start_Timestamp")), int(col(r, "End_Timestamp")), col(r, "Direction") or "?",
                   col(r, "Stream_Id", "Queue_Id") or "?"))
kern.sort()
copies.sort()
kern_by_stream = list(kern)                            # (the paired pump's kernels are read as one stream below)
# (k_dfs_pure: k_dfs and k_graph_pure as one launch, the default since round 6 — a step then has six kernels, not seven.
# k_dfs_pure_seed, round 7's paired pump: that launch with k_seed of the NEXT batch in it.  What a stream then shows
# between two k_pack is k_pack of the next batch, the paired launch, and the back and the copy of the PREVIOUS batch —
# five kernels, the span of one step of the pump all the same)
ours = ("k_pack", "k_seed", "k_dfs", "k_dfs_pure", "k_dfs_pure_seed", "k_graph_pure", "k_graph", "k_out_scan", "k_out_pack")
# The paired pump runs the steps' chain (k_pack, k_dfs_pure_seed) on one stream and their backs and copies on another,
# both FIFO: the commands are read as ONE stream, and the m-th delivery copy belongs to the m-th k_pack.
paired = any(name == "k_dfs_pure_seed" for _s, _e, name, _st in kern)
if paired:
    kern = [(s, e, name, "paired") for s, e, name, st in kern]
steps_by_stream = collections.defaultdict(list)        # stream -> list of dicts
cur = {}
for s, e, name, st in kern:
    if name not in ours:
        continue
    if name == "k_pack":
        cur[st] = {"stream": st, "start": s, "kernels": {}, "k_end": e}
        steps_by_stream[st].append(cur[st])
    step = cur.get(st)
    if step is None:
        # (round 2: k_graph_pure ran on the batch's side stream) attach it to the step in flight that started last
        live = [v for v in cur.values() if v["start"] <= s]
        step = max(live, key=lambda v: v["start"]) if live else None
        if step is None:
            continue
    step["kernels"][name] = step["kernels"].get(name, 0) + (e - s)
    step["k_end"] = max(step["k_end"], e)
d2h = [c for c in copies if "DEVICE_TO_HOST" in c[2].upper() or "D2H" in c[2].upper()]
# a delivered step: the first D2H that starts after its k_out_pack ended, before the stream's next k_pack
all_steps = sorted((st for lst in steps_by_stream.values() for st in lst), key=lambda v: v["start"])
for lst in steps_by_stream.values():
    for i, stp in enumerate(lst):
        nxt = lst[i + 1]["start"] if i + 1 < len(lst) else None
        stp["next_start"] = nxt
        if "k_out_pack" not in stp["kernels"]:
            continue
        cand = [c for c in d2h if c[0] >= stp["k_end"] - 1000 and (nxt is None or c[0] < nxt) and c[1] - c[0] > 20000]
        if cand:
            stp["d2h"] = (cand[0][0], cand[0][1])
if paired:
    big = [c for c in d2h if c[1] - c[0] > 20000]
    lst = steps_by_stream["paired"]
    # (the match is by ordinal: right when every step of the trace went through the pump's two streams.  A trace that
    # mixes in steps on the batches' own streams — fallbacks — may deliver out of that order: the counts then differ or
    # the spans come out negative, and the summary says so instead of reporting them)
    n_fused = sum(1 for _s, _e, name, _st in kern if name == "k_dfs_pure_seed")
    mismatch = len(lst) != len(big) or n_fused + 8 < len(lst)
    if mismatch:
        print("timeline_summary: %d k_pack, %d delivery copies, %d paired launches: steps and copies are NOT matched one "
              "to one, the per-step spans are unreliable" % (len(lst), len(big), n_fused), file=sys.stderr)
    for stp, c in zip(lst, big):
        stp["d2h"] = (c[0], c[1])
        stp["k_end"] = min(stp["k_end"], c[0])
        stp["next_start"] = None           # (a stream's idle time between copy and k_pack has no meaning here)
delivered = [v for v in all_steps if "d2h" in v and (paired or len(v["kernels"]) >= 6)]
# the pipelined region: the longest stretch of delivered steps whose starts are < 2 ms apart, >= 3 streams alternating
best, run = [], []
for v in delivered:
    if run and v["start"] - run[-1]["start"] > 2_000_000:
        if len(run) > len(best):
            best = run
        run = []
    run.append(v)
if len(run) > len(best):
    best = run
res = {"kernel_rows": len(kern), "copy_rows": len(copies), "delivered_steps_found": len(delivered)}
if paired:
    res["paired_pump"] = {"steps_matched_to_copies_by_order": True, "counts_match": not mismatch}
if len(best) >= 8:
    t0, t1 = best[0]["start"], max(v["d2h"][1] for v in best)
    wall = t1 - t0
    n = len(best)

    def union(iv):
        iv = sorted(iv)
        tot, ce = 0, None
        cs = None
        for s, e in iv:
            if ce is None or s > ce:
                if ce is not None:
                    tot += ce - cs
                cs, ce = s, e
            else:
                ce = max(ce, e)
        if ce is not None:
            tot += ce - cs
        return tot

    kin = [(max(s, t0), min(e, t1)) for s, e, name, st in kern if name in ours and e > t0 and s < t1]
    cin = [(max(c[0], t0), min(c[1], t1)) for c in d2h if c[1] > t0 and c[0] < t1]
    gaps = [v["next_start"] - v["d2h"][1] for v in best if v["next_start"] is not None and v["next_start"] > v["d2h"][1]]
    waits = [v["d2h"][0] - v["k_end"] for v in best]
    per_k = collections.defaultdict(list)
    for v in best:
        for k_, d in v["kernels"].items():
            per_k[k_].append(d)
    spans = [v["d2h"][1] - v["start"] for v in best]
    res.update({
        "region": {"steps": n, "streams": len({v["stream"] for v in best}), "wall_us": wall / 1e3,
                   "us_per_step": wall / 1e3 / n},
        "some_kernel_running_frac": union(kin) / wall,
        "sum_of_kernel_durations_per_step_us": sum(e - s for s, e in kin) / 1e3 / n,
        "copy_engine_busy_frac": union(cin) / wall,
        "d2h_us": {"mean": sum(e - s for s, e in cin) / max(1, len(cin)) / 1e3, "count": len(cin)},
        "step_span_us_pack_to_copy_end": {"mean": sum(spans) / n / 1e3, "max": max(spans) / 1e3},
        "copy_start_after_last_kernel_us": {"mean": sum(waits) / n / 1e3, "max": max(waits) / 1e3},
        "stream_idle_copy_end_to_next_k_pack_us": {"mean": (sum(gaps) / len(gaps) / 1e3) if gaps else None,
                                                   "max": (max(gaps) / 1e3) if gaps else None, "count": len(gaps)},
        "kernel_us_inside_pipeline": {k_: sum(v) / len(v) / 1e3 for k_, v in per_k.items()},
        "note": "kernel durations inside the pipeline are stretched by sharing the CUs with the other batches' "
                "kernels (compare profiles/*kernel_stats.csv: each kernel alone)",
    })
if paired and len(best) >= 8:
    # ---- the pump's streams one by one, inside the same region
    per_stream = collections.defaultdict(lambda: {"busy": 0, "names": collections.Counter()})
    for s, e, name, st in kern_by_stream:
        if name in ours and e > t0 and s < t1:
            per_stream[("kernels", st)]["busy"] += min(e, t1) - max(s, t0)
            per_stream[("kernels", st)]["names"][name] += 1
    for c in d2h:
        if c[1] > t0 and c[0] < t1 and c[1] - c[0] > 20000:
            per_stream[("copies", c[3])]["busy"] += min(c[1], t1) - max(c[0], t0)
            per_stream[("copies", c[3])]["names"]["delivery copy"] += 1
    res["pump_streams"] = [
        {"stream": st, "rows": kind, "queue_ids": sorted(queue_of.get(st, {"?"})) if kind == "kernels" else None,
         "carries": dict(v["names"]), "busy_us_per_step": v["busy"] / 1e3 / n}
        for (kind, st), v in sorted(per_stream.items())]
    # ---- the chain: how long after the end of the paired launch before it does a paired launch start, and how often
    # is the k_pack it needs still running at that end (the launch then waits for it: on the chain itself k_pack sits
    # in that gap by construction, on the front — KM_PUMP_FRONT — only when it came late).  Every k_pack is consumed
    # by the next k_seed or paired launch of its batch, in order: the m-th k_pack belongs to the m-th of those.
    packs = [(s, e) for s, e, name, _st in kern_by_stream if name == "k_pack"]
    users = [(s, e, name) for s, e, name, _st in kern_by_stream if name in ("k_seed", "k_dfs_pure_seed")]
    matched = len(packs) == len(users)
    gaps_all, late, after_pack, prev_end = [], [], [], None
    for (ps, pe), (s, e, name) in zip(packs, users):
        if name == "k_dfs_pure_seed" and prev_end is not None and s >= t0 and e <= t1:
            gaps_all.append(s - prev_end)
            after_pack.append(s - pe)
            if pe > prev_end:
                late.append(s - prev_end)
        prev_end = e if name == "k_dfs_pure_seed" else None      # (a run of paired steps starts behind a k_seed)
    res["chain"] = {"paired_launches_behind_a_paired_launch": len(gaps_all), "k_pack_matched_by_order": matched,
                    "gap_between_launches_us": {"mean": sum(gaps_all) / max(1, len(gaps_all)) / 1e3,
                                                "median": sorted(gaps_all)[len(gaps_all) // 2] / 1e3 if gaps_all else None,
                                                "max": max(gaps_all) / 1e3 if gaps_all else None},
                    "launch_start_after_its_k_pack_end_us": {"median": sorted(after_pack)[len(after_pack) // 2] / 1e3 if after_pack else None},
                    "launch_waited_for_k_pack": {"count": len(late), "mean_us": sum(late) / len(late) / 1e3 if late else 0.0,
                                                 "max_us": max(late) / 1e3 if late else 0.0}}
json.dump(res, open(out_path, "w"), indent=1)
print(json.dumps(res))
