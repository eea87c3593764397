"""Device-side digests of every GroupNorm output (y, statistics, gx, gskip, ggamma, gbeta) over the case table of
tests/test_hip_groupnorm_fp64.py -- every (relu, skip), cluster modes 1 and 0, through ops.group_norm_act -- and of all six
(mask, gskip) backward forms through ecm_gn3d_fwd / _bwd and ecm_gn3d_fwd_p / _bwd_p, for the library that ECM_HIP_LIB selects:
a change of host code must leave every digest as it was.
usage: gn_digest.py OUT.json                             (one process per library)
       gn_digest.py --compare PARENT.json CHANGE.json OUT.json"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

M1, M2 = 0x9E3779B97F4A7C15 - (1 << 64), 0xC2B2AE3D27D4EB4F - (1 << 64)


def digest(t):
    """two position-dependent 64-bit sums (wrapping int64 arithmetic) over the tensor's 32-bit words, on the device"""
    w = t.detach().contiguous().view(torch.int32).reshape(-1)
    a = b = 0
    step = 1 << 26
    for i in range(0, w.numel(), step):
        v = w[i:i + step].to(torch.int64)
        idx = torch.arange(i, i + v.numel(), device=v.device, dtype=torch.int64)
        a += int(((v + 1) * (idx * M1 + 1)).sum())
        b += int(((v ^ (idx * M2)) * (idx + 12345)).sum())
    return f"{a & (2**64 - 1):016x}{b & (2**64 - 1):016x}"


def compare(parent, change, dst):
    p, c = (json.load(open(f)) for f in (parent, change))
    assert p["digests"].keys() == c["digests"].keys()
    by_entry = {}
    for k in p["digests"]:
        by_entry[k.split("/")[0]] = by_entry.get(k.split("/")[0], 0) + 1
    res = {"what": "two position-dependent 64-bit sums over the 32-bit words of every tensor, computed on the device",
           "parent_abi": p["abi"], "change_abi": c["abi"], "tensors": p["tensors"], "by_entry": by_entry,
           "quantities": sorted({k.split("/")[-1] for k in p["digests"]}),
           "differing": sorted(k for k in p["digests"] if p["digests"][k] != c["digests"][k])}
    with open(dst, "w") as f:
        json.dump(res, f, indent=1)
    print(res["tensors"], "tensors,", len(res["differing"]), "differ")
    return 1 if res["differing"] else 0


def main():
    if sys.argv[1] == "--compare":
        return compare(*sys.argv[2:5])
    import ecm_amd as ecm
    import test_hip_groupnorm_fp64 as T
    out = {}
    n = 0
    combos = [(False, False), (False, True), (True, False), (True, True)]
    for name, shape in T.CASES.items():
        for relu, skip in combos:
            x, gm, bt, sk, gy = T._data(shape, skip, T._seed(name, relu, skip))
            for mode in ((1,) if name in T.PRODUCTION else (1, 0)):
                with T.cluster_mode(ecm, mode):
                    q = T._hip(ecm, x, gm, bt, sk, relu, gy)
                for k, v in q.items():
                    out[f"ops/{name}/relu{int(relu)}/skip{int(skip)}/mode{mode}/{k}"] = digest(v)
                    n += 1
                del q
            del x, sk, gy
        torch.cuda.empty_cache()
        print("case", name, "done", flush=True)
    lib = ecm.ops._lib
    import ctypes as C
    for kind, shape in T.ABI_SHAPES.items():
        # every (relu, mask source, gskip) the C ABI accepts: relu off -> mask 0; relu on, y given -> 1; relu on, y NULL -> 2
        for relu, use_y, want_gskip in [(r, u, g) for r in (False, True) for u in ((False, True) if r else (False,)) for g in (False, True)]:
            skip = use_y
            x, gm, bt, sk, gy = T._data(shape, skip, T._seed("abi", kind, relu, use_y, want_gskip))
            keep = torch.empty(lib.query("ecm_gn3d_cluster_bytes", shape[0]), dtype=torch.uint8, device="cuda")
            lib.call("ecm_gn3d_cluster_preset", ecm.ops._p(keep), C.c_longlong(keep.numel()), ecm.ops._stream())
            for mode in (1, 0):
                with T.cluster_mode(ecm, mode):
                    for entry, kp in (("stateless", None), ("_p", keep)):
                        q = T._abi(ecm, kp, x, gm, bt, sk, relu, gy, use_y, want_gskip)
                        for k, v in q.items():
                            out[f"abi/{kind}/relu{int(relu)}/y{int(use_y)}/gskip{int(want_gskip)}/mode{mode}/{entry}/{k}"] = digest(v)
                            n += 1
        print("abi", kind, "done", flush=True)
    ecm.ops.check_async_errors()
    res = {"lib": os.environ.get("ECM_HIP_LIB", "default"), "abi": lib.query("ecm_abi_version"), "tensors": n, "digests": out}
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("digests:", n)
    return 0


if __name__ == "__main__":
    sys.exit(main())
