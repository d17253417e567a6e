"""Bit identity of the small layers' GEMM kernels between two builds of the library (one selected per
process with PN2_LIB_SUFFIX): every output of mlp_gemm_forward_small (with and without bias, with and
without the weight image), mlp_gemm_dgrad on its small path, mlp_gemm_backward_small and
mlp_gemm_wgrad (direct kernel) on the same seeded inputs, at the shapes of
tests/test_small_gemm_tail.py -- as SHA-256 digests of the raw bytes.

    PN2_LIB_SUFFIX=_par python tools/small_tail_identity.py run parent.json
    python tools/small_tail_identity.py run new.json
    python tools/small_tail_identity.py compare parent.json new.json [out.json]
    python tools/small_tail_identity.py dumps DIR_A DIR_B        (bench.py --dump-outputs directories)
"""
import hashlib
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 64, 64, 64), (2, 79, 128, 100), (3, 33, 70, 37), (1, 20, 259, 8), (8, 128, 128, 256),
          (8, 256, 256, 1024), (8, 256, 256, 2048)]


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run(out):
    import torch
    sys.path.insert(0, ROOT)
    importlib.import_module("3dioumatch_amd")
    K = importlib.import_module("pointnet2._mlp_ext")
    dev = "cuda:0"
    res = {}
    for b, m, k, r in SHAPES:
        g = torch.Generator().manual_seed(b * 100003 + m * 1009 + k * 31 + r)
        rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
        ru = lambda *s: torch.rand(*s, generator=g).to(dev)   # noqa: E731
        w, x, bias = rn(m, k) / k ** 0.5, rn(b, k, r), rn(m)
        xc = (ru(k) + 0.5, rn(k) * 0.3)
        y, dz = rn(b, m, r), rn(b, m, r)
        coef = torch.stack([ru(m) + 0.5, rn(m) * 0.1, rn(m) * 0.1], dim=1).contiguous()
        fly = (y, dz, ru(m) + 0.5, rn(m) * 0.3, rn(m) * 0.2, ru(m) + 0.5, coef)
        ns = 16 if r % 16 == 0 else (4 if r % 4 == 0 else r)
        argmax = torch.randint(0, ns, (b, m, r // ns), generator=g, dtype=torch.int32).to(dev)
        pooled = (y.view(b, m, r // ns, ns), rn(b, m, r // ns), argmax) + fly[2:]
        images = K.WeightImages([w])
        images.refresh()
        row = {}
        for image in (False, True):
            with K.weight_images(images if image else None):
                for cn, coeff in (("direct", None), ("bnrelu", xc)):
                    for bn, bv in (("", None), ("+bias", bias)):
                        row["forward %s%s image=%d" % (cn, bn, image)] = digest(K.gemm_forward(w, x, coeff, bv))
                    if r >= 32:
                        dx, dw = K.gemm_backward_small(w, x, coeff, dy=dz)
                        row["pair dy %s image=%d dx" % (cn, image)] = digest(dx)
                        row["pair dy %s image=%d dw" % (cn, image)] = digest(dw)
        for gn, grad in (("dy", dict(dy=dz)), ("fly", dict(fly=fly)), ("pooled", dict(pooled=pooled))):
            row["dgrad " + gn] = digest(K.gemm_dgrad(w, **grad))
            if gn == "pooled":
                continue
            for cn, coeff in (("direct", None), ("bnrelu", xc)):
                row["wgrad %s %s" % (gn, cn)] = digest(K.gemm_wgrad(m, k, x, coeff, **grad))
                if r >= 32 and gn == "fly":
                    dx, dw = K.gemm_backward_small(w, x, coeff, fly=fly)
                    row["pair fly %s dx" % cn] = digest(dx)
                    row["pair fly %s dw" % cn] = digest(dw)
        res["x".join(map(str, (b, m, k, r)))] = row
    torch.cuda.synchronize()
    json.dump({"lib_suffix": os.environ.get("PN2_LIB_SUFFIX", ""), "digests": res}, open(out, "w"), indent=1)
    print("wrote %s: %d tensors" % (out, sum(len(v) for v in res.values())))


def compare(a, b, out=None):
    da, db = json.load(open(a))["digests"], json.load(open(b))["digests"]
    differ = [s + " / " + n for s in da for n in da[s] if db.get(s, {}).get(n) != da[s][n]]
    differ += [s + " / " + n for s in db for n in db[s] if n not in da.get(s, {})]
    total = sum(len(v) for v in da.values())
    verdict = {"tensors": total, "differ": differ, "bit_equal": not differ}
    print(json.dumps(verdict))
    if out:
        json.dump(verdict, open(out, "w"), indent=1)
    return 0 if not differ else 1


def dumps(a, b):
    import numpy as np
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    differ = []
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            differ.append(n + " (missing)")
        elif n.endswith(".npy"):
            if np.load(pa).tobytes() != np.load(pb).tobytes():
                differ.append(n)
        elif open(pa, "rb").read() != open(pb, "rb").read():
            differ.append(n)
    print(json.dumps({"arrays": len(names), "differ": differ, "bit_equal": not differ}))
    return 0 if not differ else 1


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    elif sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:5]))
    else:
        sys.exit(dumps(sys.argv[2], sys.argv[3]))
