"""Per-shape durations of the NT launches of ONE posterior heat map per precision mode (GPU box).
   SLN_NT_LOG=1 makes the launchers print a line per launch; this script runs itself under rocprofv3 --kernel-trace (a run of its
   own: no counters, no other tracing), then joins the NT dispatches of the trace - in order - with those lines.
       python tools/lab/heatmap_nt_by_shape.py [samples] [out dir]
   TF/s counts 2 M N K per launch; "mfma" is the share of the fp16 MFMA peak (2 500 TF/s dense) counting every product issued
   (x3 in f16x3), or of the fp32 MFMA peak (157.3 TF/s) for the fp32 kernels."""
import csv, glob, importlib, os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
MODES = ("fp32", "f16x3", "f16")


def child(n):
    import torch
    M = importlib.import_module("3d_sln_amd.host.Sg2ScVAE_model"); syn = importlib.import_module("3d_sln_amd.host.synthetic")
    S = importlib.import_module("3d_sln_amd.host.sampling")
    torch.manual_seed(0)
    model = M.Sg2ScVAEModel(vocab=syn.default_vocab(), batch_size=1, train_3d=True, decoder_cat=True, embedding_dim=64, gconv_mode='feedforward',
                            gconv_num_layers=5, mlp_normalization='batch', vec_noise_dim=0, layout_noise_dim=32, use_AE=False).cuda().eval()
    objs5 = ["bed", "desk", "cabinet", "chair", "lamp"]
    rels5 = [("bed", "behind", "desk"), ("cabinet", "left of", "bed"), ("chair", "left of", "desk"), ("lamp", "on", "desk")]
    mean = torch.zeros(64, dtype=torch.float64); cov = torch.eye(64, dtype=torch.float64)
    for rep in range(3):
        for m in MODES:
            if rep == 2:
                sys.stderr.write("NTLOG BEGIN %s\n" % m); sys.stderr.flush()
            S.heatmap_from_words(model, objs5, rels5, mean, cov, num_iter=n, chunk=n, precision=m)
            torch.cuda.synchronize()
            if rep == 2:
                sys.stderr.write("NTLOG END %s\n" % m); sys.stderr.flush()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    if os.environ.get("NT_CHILD"):
        return child(n)
    out = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else "/tmp/heatmap_nt_by_shape"
    subprocess.run(["rm", "-rf", out])
    env = dict(os.environ, NT_CHILD="1", SLN_NT_LOG="1")
    r = subprocess.run(["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "t", "--", sys.executable,
                        os.path.abspath(__file__), str(n)], env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stdout.write(r.stdout[-2000:]); sys.stderr.write(r.stderr[-4000:])
        return r.returncode
    log = [l for l in r.stderr.split("\n") if l.startswith("NTLOG")]
    shapes_all = [l for l in log if "M=" in l]
    f = glob.glob(out + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda x: int(x["Start_Timestamp"]))
    nt = [x for x in rows if re.search(r"gemm_nt(_small|16|_half)?_kernel", x["Kernel_Name"])]
    assert len(nt) == len(shapes_all), (len(nt), len(shapes_all))
    pos = 0
    spans = {}
    for l in log:                                   # positions of each mode's timed heat map in the launch sequence
        if l.startswith("NTLOG BEGIN"):
            cur, first = l.split()[2], pos
        elif l.startswith("NTLOG END"):
            spans[cur] = (first, pos)
        elif "M=" in l:
            pos += 1
    for mode in MODES:
        a, b = spans[mode]
        agg, tot = {}, 0.0
        for l, x in zip(shapes_all[a:b], nt[a:b]):
            us = (int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3
            m = dict(kv.split("=") for kv in l.split()[1:])
            kn = re.sub(r"void \(anonymous namespace\)::|\(GemmNTArgs.*", "", x["Kernel_Name"])
            key = (int(m["M"]), int(m["N"]), int(m["K"]), m["amode"], m["nseg"], int(m.get("half", 0)), kn)
            agg.setdefault(key, []).append(us)
        print("== %s, %d layouts" % (mode, n))
        print("%8s %5s %5s  am sg  %-46s %3s %9s %8s %6s" % ("M", "N", "K", "kernel", "n", "avg us", "TF/s", "mfma"))
        for k, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
            avg = sum(v) / len(v); fl = 2.0 * k[0] * k[1] * k[2]; tot += sum(v)
            tf = fl / avg / 1e6
            frac = tf * k[5] / 2500.0 if k[5] else tf / 157.3
            print("%8d %5d %5d  %s  %s  %-46s %3d %9.1f %8.1f %6.3f" % (k[0], k[1], k[2], k[3], k[4], k[6], len(v), avg, tf, frac))
        print("NT launches of one heat map: %d, %.3f ms" % (b - a, tot / 1e3))
    return 0


if __name__ == "__main__":
    sys.exit(main())
