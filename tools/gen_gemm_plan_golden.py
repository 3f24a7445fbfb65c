#!/usr/bin/env python3
"""Record which tile variant and K-split the forward gives every GEMM shape: tests/golden/gemm_plan.json.

    python tools/gen_gemm_plan_golden.py            # rewrite the file from the built library
    python tools/gen_gemm_plan_golden.py --print    # the same JSON on stdout (tests/test_host_cpu.py compares it with the file)

Needs no GPU (jat_model_create and jat_k_gemm_plan are host code).  The JAT_* variables that steer the chooser must be unset
(CHOOSER_ENV; they are read once per process).

The committed file was recorded from commit 5e2fbc3, the last one that planned inside jat_api.cpp, with only
tools/gemm_plan_parent_wrapper.patch applied (it adds jat_k_gemm_plan as a wrapper over that commit's pick_variant / resid_split /
qkv_split / patch_split): `git checkout 5e2fbc3 && git apply <this tree>/tools/gemm_plan_parent_wrapper.patch && make -C
jatsr-just-audio-transformer-super-solution_amd/csrc`, then run this script with JAT_LIB_PATH pointing at that libjat_hip.so.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "gemm_plan.json")
CHOOSER_ENV = ("JAT_EPI_PIPE", "JAT_KPAIR", "JAT_PERSIST", "JAT_KPAIR_SPLIT", "JAT_GEMM_VARIANT", "JAT_GEMM_VARIANTS",
               "JAT_QKV_SPLIT", "JAT_PATCH_SPLIT")

# rows: the product's buckets, both sides of every threshold of the planner, every multiple of 224 up to 7168, ragged values
MS = sorted(set([240, 345, 690, 1380, 2760, 3584, 7168, 9660, 14336] + [1535, 1536, 2047, 2048, 2304, 2305, 4096, 4097] +
                list(range(224, 7168 + 1, 224)) + [1000, 1035, 4500]))
MODELS = {
    # v3mod2: qkv, out_proj, fc1, fc2, first patch-embed Linear (CFG-shared / plain), second one, final layer, adaLN
    "v3mod2": dict(cfg=dict(input_channels=1024, cond_channels=1024, patch_len=4, hidden_size=1280, depth=28, num_q_heads=20,
                            num_kv_heads=4, bottleneck_dim=512, mlp_hidden=5120, norm_mode=0),
                   NK=[(1792, 1280), (1280, 1280), (5120, 1280), (1280, 5120), (512, 4096), (512, 8192), (1280, 512), (4096, 1280),
                       (6 * 1280 * 28, 1280)]),
    # other dimensions: D % 160 != 0
    "d512": dict(cfg=dict(input_channels=256, cond_channels=256, patch_len=4, hidden_size=512, depth=4, num_q_heads=8,
                          num_kv_heads=2, bottleneck_dim=256, mlp_hidden=2048, norm_mode=0),
                 NK=[(768, 512), (512, 512), (2048, 512), (512, 2048), (256, 1024), (256, 2048), (512, 256), (1024, 512),
                     (6 * 512 * 4, 512)]),
}
SWITCHES = {"default": {}, "qkv_split=0": {"qkv_split": 0}, "patch_split=0": {"patch_split": 0}}


def collect():
    from jatsr_amd import _lib as L
    lib = L.lib()
    out = {"_layout": "plans[model][switches][site 0..4][folding 0/1][i of NK][j of M] = [variant, ksplit]",
           "M": MS, "wave_n": [lib.jat_k_gemm_wave_n(v) for v in range(40)], "NK": {}, "plans": {}}
    v, k = C.c_int32(), C.c_int32()
    for name, spec in MODELS.items():
        out["NK"][name] = [list(nk) for nk in spec["NK"]]
        out["plans"][name] = {}
        for sw_name, sw in SWITCHES.items():
            cfg = L.JatConfig(*[spec["cfg"][n] for n, _ in L.JatConfig._fields_])
            h = C.c_void_p()
            L.check(lib.jat_model_create(C.byref(cfg), C.byref(h)))
            for key, val in sw.items():
                L.check(lib.jat_model_set_switch(h, key.encode(), val))
            table = []
            for site in range(5):
                per_fold = []
                for folding in (0, 1):
                    per_nk = []
                    for N, K in spec["NK"]:
                        row = []
                        for M in MS:
                            L.check(lib.jat_k_gemm_plan(h, site, M, N, K, folding, C.byref(v), C.byref(k)))
                            row.append([v.value, k.value])
                        per_nk.append(row)
                    per_fold.append(per_nk)
                table.append(per_fold)
            out["plans"][name][sw_name] = table
            lib.jat_model_destroy(h)
    return out


def dumps(d):
    return json.dumps(d, separators=(",", ":"))


if __name__ == "__main__":
    bad = [n for n in CHOOSER_ENV if n in os.environ]
    if bad:
        sys.exit(f"unset {', '.join(bad)} first: they change the plans")
    if "--print" in sys.argv[1:]:
        print(dumps(collect()))
    else:
        with open(PATH, "w") as f:
            f.write(dumps(collect()) + "\n")
        print(f"wrote {PATH}")
