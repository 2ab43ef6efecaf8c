"""End-of-flood figures from a rocprofv3 kernel trace CSV of the bench, averaged over the last 20 steps (threshold to threshold):
round launches per step, durations of the last four rounds, idle time between rounds, gap last round -> mask write, gap mask
write -> k_mc_count, step length."""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
idx = [i for i, r in enumerate(rows) if "k_threshold16" in r["Kernel_Name"]]
steps = list(zip(idx[:-1], idx[1:]))[-20:]
acc = {"rounds": [], "idle_between_rounds": [], "max_idle_between_rounds": [], "gap_round_to_write": [], "write_dur": [],
       "gap_write_to_count": [], "step": [], "last4": []}
for i0, i1 in steps:
    ks = rows[i0:i1]
    S = lambda r: int(r["Start_Timestamp"]) / 1e3
    E = lambda r: int(r["End_Timestamp"]) / 1e3
    rd = [r for r in ks if "k_flood_round_list" in r["Kernel_Name"]]
    wr = [r for r in ks if "k_flood_apply" in r["Kernel_Name"]]
    mc = [r for r in ks if "k_mc_count" in r["Kernel_Name"]]
    if not rd or not wr or not mc:
        continue
    gaps = [S(b) - E(a) for a, b in zip(rd[:-1], rd[1:])]
    acc["rounds"].append(len(rd))
    acc["idle_between_rounds"].append(sum(gaps))
    acc["max_idle_between_rounds"].append(max(gaps) if gaps else 0.0)
    acc["gap_round_to_write"].append(S(wr[0]) - E(rd[-1]))
    acc["write_dur"].append(E(wr[0]) - S(wr[0]))
    acc["gap_write_to_count"].append(S(mc[0]) - E(wr[0]))
    acc["step"].append(S(rows[i1]) - S(rows[i0]))
    acc["last4"].append([round(E(r) - S(r), 1) for r in rd[-4:]])
n = len(acc["rounds"])
print("steps", n)
for k, v in acc.items():
    if k != "last4":
        print("%-26s mean %7.2f  min %7.2f  max %7.2f" % (k, sum(v) / n, min(v), max(v)))
l4 = acc["last4"]
print("last four rounds' durations, mean:", [round(sum(x[j] for x in l4 if len(x) == 4) / max(1, sum(1 for x in l4 if len(x) == 4)), 2) for j in range(4)])
print("all rounds of the last step: ", [round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, 1) for r in rows[steps[-1][0]:steps[-1][1]] if "k_flood_round_list" in r["Kernel_Name"]])
