#!/usr/bin/env python3
"""The parity margins of the natural-gradient kernels for actors with three and four hidden layers (csrc/pds_npg_deep.hip), per
case of tests/npg_deep_cases.py, measured on the device in one process:

  Fisher product  per parameter tensor: rho of torch's float32 double backward (the reference side of the bar: its table-wide
                  maximum per tensor position is npg_deep_cases.F32_AUTOGRAD_RHO), rho of the kernel, and the kernel's error / bar
                  under the rule of npg_deep_cases.fvp_bars (8 x the float32 rho, within [2^-21, 2e-5]; whole vector 2e-5)
  line search     error / bar of the three sums under npg_cases.ls_merged_bars, worst over the finite candidates

  python profiles/tools/npg_deep_margins.py > profiles/npg_deep_parity_margins.txt"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import npg_cases as nc  # noqa: E402
import npg_deep_cases as ndc  # noqa: E402
from phoenix_drone_simulation_amd.fused import FusedMLP  # noqa: E402

DEV = "cuda:0"
POSITIONS = ("W_first", "b_first", "W_inner", "b_inner", "W_out", "b_out")


def main():
    assert torch.cuda.is_available(), "npg_deep_margins.py needs a HIP device"
    print(f"# csrc/pds_npg_deep.hip against the float64 references of tests/npg_deep_cases.py, {torch.cuda.get_device_name(0)}")
    print("# Fisher product: rho = |result - ref_fvp| / |ref_fvp| per tensor, for torch's float32 double backward (f32) and for the")
    print("# kernel (hip); err/bar = the kernel's error over the bar of npg_deep_cases.fvp_bars, worst over the tensors and the whole vector")
    f32_max = {p: 0.0 for p in POSITIONS}
    hip_max = {p: 0.0 for p in POSITIONS}
    worst_fvp = 0.0
    for c in ndc.FVP_CASES:
        i = ndc.make_inputs(c, DEV)
        net, x, index, xs, log_std, v = (i[k] for k in ("net", "x", "index", "xs", "log_std", "v"))
        fm = FusedMLP(net, c.act, npg_deep=True)
        got = fm.fisher_vector_product(x, v, log_std, 0.0, index=index)
        want = nc.ref_fvp(net, xs, log_std, v)
        f32 = ndc.tensor_rho(nc.fvp_autograd(net, xs, log_std, v, torch.float32), want, c)
        hip = ndc.tensor_rho(got, want, c)
        cancel = nc.ref_fvp_dense(net, xs, log_std, v, ndc.cancel_depth(c))[1] if c.B <= ndc.DENSE_MAX else None
        rank_one = ndc.cancel_applies(c)
        live = None if rank_one else {k: (r if math.isfinite(r) else 0.0) for k, r in f32.items()}
        margins = ndc.fvp_margins(c, got, want, cancel, live)
        worst_fvp = max(worst_fvp, max(margins.values()))
        zero = [n for n, sl in ndc.slices(c).items() if float(torch.norm(want[sl])) == 0.0]
        if not rank_one:  # (the rank-one cases' error is the cancellation term's: left out of the maxima)
            for name in ndc.tensors(c):
                p = ndc.position(name, c)
                if math.isfinite(f32[name]):
                    f32_max[p] = max(f32_max[p], f32[name])
                if math.isfinite(hip[name]):
                    hip_max[p] = max(hip_max[p], hip[name])
        print(f"{ndc.case_id(c):52s} err/bar {max(margins.values()):6.3f} (whole {margins['whole']:.3f})"
              + (" rank-one" if rank_one else "") + (f" exactly zero: {' '.join(zero)}" if zero else ""))
        print("    f32 " + " ".join(f"{k} {r:.2e}" for k, r in f32.items()))
        print("    hip " + " ".join(f"{k} {r:.2e}" for k, r in hip.items()))
        print("    err/bar " + " ".join(f"{k} {r:.3f}" for k, r in margins.items() if k != "whole"))
    print(f"# Fisher product: worst err/bar {worst_fvp:.3f} over {len(ndc.FVP_CASES)} cases (with the F32_AUTOGRAD_RHO the module holds now)")
    print("# table-wide maxima of the float32-autograd rho per tensor position (-> npg_deep_cases.F32_AUTOGRAD_RHO):")
    print("F32_AUTOGRAD_RHO = {" + ", ".join(f'"{p}": {f32_max[p]:.3e}' for p in POSITIONS) + "}")
    print("# the kernel's own maxima per tensor position, and their ratio to the bar 8 x max(f32 maximum, 2^-21 / 8) capped at 2e-5:")
    for p in POSITIONS:
        bar = min(max(ndc.TENSOR_FACTOR * f32_max[p], ndc.TENSOR_FLOOR), ndc.FVP_REL)
        print(f"#   {p:8s} hip {hip_max[p]:.3e}  bar {bar:.3e}  ratio {hip_max[p] / bar:.3f}")
    print("# line search: err / merged bar of (sum ratio adv, sum KL, sum ratio), worst over the finite candidates of npg_cases.LS_FRACS")
    worst_ls = [0.0, 0.0, 0.0]
    for c in ndc.LS_CASES:
        i = ndc.make_inputs(c, DEV)
        fm = FusedMLP(i["net"], c.act, npg_deep=True)
        fracs = torch.tensor(ndc.LS_FRACS, dtype=torch.float32, device=DEV)
        mu_old = fm.forward(i["x"])
        args = (i["x"], i["act"], i["adv"], i["logp_old"], mu_old, i["log_std"])
        out = fm.surrogate_kl(i["s"], fracs, *args).cpu()
        w = [0.0, 0.0, 0.0]
        for j, f in enumerate(ndc.LS_FRACS):
            if not math.isfinite(f):
                continue
            ref = nc.ref_ls(i["net"], i["theta"] + f * i["s"], *args)
            bars = nc.ls_merged_bars(ref, c.B, c.d_out)
            errs = [abs(float(out[j, 0]) - ref["ra"]), abs(float(out[j, 1]) - ref["kl"]), abs(float(out[j, 3]) - ref["rs"])]
            w = [max(a, e / b) for a, e, b in zip(w, errs, bars)]
        worst_ls = [max(a, b) for a, b in zip(worst_ls, w)]
        print(f"{ndc.case_id(c):52s} err/bar " + " ".join(f"{r:.4f}" for r in w))
    print("# line search: worst err/bar " + " ".join(f"{r:.4f}" for r in worst_ls) + f" over {len(ndc.LS_CASES)} cases")


if __name__ == "__main__":
    main()
