"""rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE counter_collection CSVs of a bench.py run -> profiles/r02_pmc.json:
HBM bytes per launch of the two frame-embedding kernels and HBM bytes per STEP of the encoder-layer family
(every launch between the embedding LayerNorm and the final norm, forward + backward).
Correction per MI355X_MICROARCH.md (HBM section): bytes = (2 * FETCH_SIZE + WRITE_SIZE) * 1024 on gfx950 (FETCH_SIZE counts the
128-B requests of wide streaming reads at 64 B; the 8-byte accesses of the fused blocks are not separately calibrated: the
figure is an upper estimate for them).
    python scripts/pmc_summary_r02.py fetch.csv write.csv <per_gpu_batch> <steps profiled> out.json"""
import csv, json, sys
from collections import defaultdict

LAYER_KERNELS = ("attn_block_fwd_kernel", "mlp_block_fwd_kernel", "mlp_block_bwd_kernel", "mlp_block_bwd8_kernel", "attn_out_bwd_kernel", "qkv_bwd_kernel", "attn_bwd_fast", "attn_fwd_fast",
                 "rowstream_kernel", "wavestream_kernel", "wgrad_dma_kernel", "ln_bwd_vec", "ln_fwd_vec", "slab_reduce",
                 "affine_fixup_kernel")


def collect(path, counter):
    per = defaultdict(list)
    with open(path) as f:
        for row in csv.DictReader(f):
            if row["Counter_Name"] == counter:
                per[row["Kernel_Name"]].append(float(row["Counter_Value"]))
    return per


def main(fetch_csv, write_csv, batch, steps, out):
    fe, wr = collect(fetch_csv, "FETCH_SIZE"), collect(write_csv, "WRITE_SIZE")
    res = {"command": "rocprofv3 --pmc FETCH_SIZE (pass 1) / --pmc WRITE_SIZE (pass 2) --kernel-trace --output-format csv -- python3 "
                      "bench.py --full --steps %d --warmup 0 --no-cpu-baseline --no-extras (bf16, per-GPU batch %d)" % (steps, batch),
           "correction": "bytes = (2 * FETCH_SIZE + WRITE_SIZE) * 1024 (MI355X_MICROARCH.md, HBM section)",
           "per_gpu_batch": batch, "steps": steps, "kernels": {}, "layer_kernels": {}}
    for tag, pat in (("embed_fwd", "embed_fwd"), ("embed_wgrad", "embed_wgrad")):
        names = [k for k in fe if pat in k]
        if not names:
            continue
        k = max(names, key=lambda n: sum(fe[n]))
        f = fe[k][1:] or fe[k]
        w = wr.get(k, [0.0])[1:] or wr.get(k, [0.0])
        fa, wa = sum(f) / len(f), sum(w) / len(w)
        res["kernels"][tag] = {"kernel": k, "launches": len(f), "FETCH_SIZE_KB_avg": round(fa, 1), "WRITE_SIZE_KB_avg": round(wa, 1),
                               "hbm_bytes_per_launch": int((2 * fa + wa) * 1024)}
    total = 0.0
    for k in fe:
        if any(p in k for p in LAYER_KERNELS):
            b = (2 * sum(fe[k]) + sum(wr.get(k, [0.0]))) * 1024 / steps
            short = k.replace("(anonymous namespace)::", "").replace("void ", "")[:70]
            res["layer_kernels"][short] = {"launches_per_step": round(len(fe[k]) / steps, 1), "hbm_bytes_per_step": int(b)}
            total += b
    res["layers_hbm_bytes_per_step"] = int(total)
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({"kernels": res["kernels"], "layers_hbm_bytes_per_step": res["layers_hbm_bytes_per_step"]}, indent=1))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
