"""Which hardware queue each rollout chain ran on (rocprofv3 --kernel-trace csv of scratch/rollout_pipe.py): per stream with a rollout
chain the Queue_Id histogram, and how often a chain's first kernel followed ANOTHER chain's last kernel on the same queue
(profiles/rollout_lanes.md).  python scratch/lane_queues.py <rocprofv3 output directory>"""
import csv, glob, sys, collections
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
rows = list(csv.DictReader(open(f)))
print("columns:", list(rows[0].keys()))
print("kernels:", len(rows))
if "Stream_Id" not in rows[0]:
    q = collections.Counter(r["Queue_Id"] for r in rows if ("heads_sample" in r["Kernel_Name"]))
    print("no Stream_Id column; heads_sample kernels per Queue_Id:", dict(q))
    sys.exit(0)
by = collections.defaultdict(list)
for r in rows:
    by[r["Stream_Id"]].append(r)
print("| Stream_Id | kernels | heads_sample | Queue_Id: kernels |")
print("|---|---|---|---|")
chains = []
for k, v in sorted(by.items(), key=lambda kv: int(kv[0])):
    hs = sum(1 for r in v if ("heads_sample" in r["Kernel_Name"]))
    q = collections.Counter(r["Queue_Id"] for r in v)
    print(f"| {k} | {len(v)} | {hs} | {dict(q)} |")
    if hs > 200:
        chains.append(k)
print("streams with a rollout chain:", chains)
byq = collections.defaultdict(list)
for r in rows:
    if r["Stream_Id"] in chains:
        byq[r["Queue_Id"]].append(r)
tot = other = tight = 0
waits = []
for q, v in byq.items():
    v.sort(key=lambda r: int(r["Start_Timestamp"]))
    for i in range(1, len(v)):
        r, p = v[i], v[i - 1]
        if "conv1_pool_fwd" not in r["Kernel_Name"]:
            continue
        tot += 1
        if p["Stream_Id"] != r["Stream_Id"] and ("heads_sample" in p["Kernel_Name"]):
            other += 1
            gap = (int(r["Start_Timestamp"]) - int(p["End_Timestamp"])) / 1e3
            waits.append(gap)
            if gap < 10.0:
                tight += 1
print(f"conv1_pool_fwd launches of the chains: {tot}; preceded on their queue by ANOTHER chain's heads_sample: {other}; "
      f"of those started within 10 us of its end: {tight}")
if waits:
    waits.sort()
    print(f"gap after the other chain's heads_sample, us: median {waits[len(waits) // 2]:.1f}, p10 {waits[len(waits) // 10]:.1f}, p90 {waits[9 * len(waits) // 10]:.1f}")
# step period of each chain (last 200 steps)
for k in chains:
    v = sorted((r for r in by[k] if ("heads_sample" in r["Kernel_Name"])), key=lambda r: int(r["End_Timestamp"]))
    print(f"stream {k}: step period {(int(v[-1]['End_Timestamp']) - int(v[-201]['End_Timestamp'])) / 200 / 1e3:.1f} us")
