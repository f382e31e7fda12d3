"""rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE counter_collection CSVs -> per-launch HBM bytes of the two frame-embedding kernels.
Correction per MI355X_MICROARCH.md (HBM section): bytes = (2 * FETCH_SIZE + WRITE_SIZE) * 1024 on gfx950."""
import csv, json, sys
from collections import defaultdict

def collect(path, counter):
    per = defaultdict(list)
    with open(path) as f:
        for row in csv.DictReader(f):
            if row["Counter_Name"] == counter:
                per[row["Kernel_Name"]].append(float(row["Counter_Value"]))
    return per

def main(fetch_csv, write_csv, batch, out):
    fe, wr = collect(fetch_csv, "FETCH_SIZE"), collect(write_csv, "WRITE_SIZE")
    res = {"command": "rocprofv3 --pmc FETCH_SIZE (pass 1) / --pmc WRITE_SIZE (pass 2) --kernel-trace --output-format csv -- python3 "
                      "bench.py --full --steps 4 --warmup 3 --no-cpu-baseline (bf16, per-GPU batch %d)" % batch,
           "correction": "MI355X_MICROARCH.md HBM section: bytes = (2 * FETCH_SIZE + WRITE_SIZE) * 1024 (gfx950 FETCH_SIZE counts the "
                         "128-B requests of wide streaming reads at 64 B)",
           "per_gpu_batch": batch, "kernels": {}}
    for tag, pat in (("embed_fwd", "embed_fwd"), ("embed_wgrad", "embed_wgrad")):
        names = [k for k in fe if pat in k]
        if not names:
            continue
        k = max(names, key=lambda n: sum(fe[n]))
        f = fe[k][1:] or fe[k]            # drop the cold first launch
        w = wr.get(k, [0.0])[1:] or wr.get(k, [0.0])
        fa, wa = sum(f) / len(f), sum(w) / len(w)
        res["kernels"][tag] = {"kernel": k, "launches": len(f), "FETCH_SIZE_KB_avg": round(fa, 1), "WRITE_SIZE_KB_avg": round(wa, 1),
                               "hbm_bytes_per_launch": int((2 * fa + wa) * 1024)}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["kernels"], indent=1))

if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4])
