#!/usr/bin/env python3
"""Measures, on the device, the units behind the bars of tests/test_gpu_ddpg_broad_kernels.py and
tests/test_gpu_ddpg_broad_trainer.py, and the kernels' own errors beside them.

For every case of tests/ddpg_broad_cases.py and every quantity (the six gradient tensors of the policy gradient and of the value
gradient, sum Q, the sum of squared errors, the forward output, the Bellman target): the error of the kernels of
include/pds_mlp_broad.h against float64 autograd, and the error of torch's own float32 arithmetic against the same float64, in
the measure that module states.  The unit of a quantity is the largest float32-torch error over the table.  The same for the
parameters after three DDPGTrainer updates at (400, 300).  Nothing is asserted here.

  python profiles/tools/ddpg_broad_margins.py --out profiles/ddpg_broad_parity_margins.txt
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ddpg_broad_cases as bc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ddpg_broad_margins.py needs a HIP device"
    out = open(args.out, "w") if args.out else sys.stdout
    print(f"# kernels of include/pds_mlp_broad.h against float64 autograd, {torch.cuda.get_device_name(0)}; measure and case table: "
          "tests/ddpg_broad_cases.py", file=out)
    print("# per case and quantity: kernel error | float32-torch error (both against float64)", file=out)
    unit = {k: 0.0 for k in bc.QUANTITIES}
    worst = {k: 0.0 for k in bc.QUANTITIES}
    for c in bc.CASES:
        m = bc.measure(c)
        print(bc.case_id(c), file=out)
        for k in bc.QUANTITIES:
            print(f"    {k:12s} {m[k][0]:.3e} | {m[k][1]:.3e}", file=out)
            unit[k] = max(unit[k], m[k][1])
            worst[k] = max(worst[k], m[k][0])
        out.flush()
    print("# unit = the largest float32-torch error over the table; kernel = the largest kernel error; bar = max(4 units, 2e-6)", file=out)
    print("KERNEL_UNITS = {", file=out)
    for k in bc.QUANTITIES:
        print(f'    "{k}": {unit[k]:.3e},  # kernel {worst[k]:.3e} = {worst[k] / max(4 * unit[k], bc.FLOOR):.3f} of the bar', file=out)
    print("}", file=out)
    # the trainer: three updates at (400, 300), mini-batch 128
    idx = bc.trainer_indices()
    ta = bc.trainer(False, False)
    state0 = {k: v.detach().clone() for k, v in ta.ac.state_dict().items()}
    p64 = bc.float64_updates(ta, state0, idx)
    p32 = bc.updated(ta, idx)
    tb = bc.trainer(True, True, state=state0)
    assert tb.fused and tb.broad and not ta.fused
    pf = bc.updated(tb, idx)
    print("# DDPGTrainer, Hover, 64 envs, (400, 300), three updates of 128 rows from one state_dict: parameter error against the "
          "float64 trainer, fused (broad_fused=True) | float32 autograd (fused=False)", file=out)
    print("TRAINER_UNITS = {", file=out)
    for k in p64:
        e32, ef = bc.tensor_error(p32[k], p64[k]), bc.tensor_error(pf[k], p64[k])
        print(f'    "{k}": {e32:.3e},  # fused {ef:.3e} = {ef / max(4 * e32, bc.FLOOR):.3f} of the bar', file=out)
    print("}", file=out)
    out.flush()


if __name__ == "__main__":
    main()
