#!/usr/bin/env python3
"""The parity margins of the deep-MLP kernels, per case, from the junit report of tests/test_gpu_mlp_deep.py (its `margin` and
`bar` properties: the ratio to the bar that applied, and which side of the rule of tests/mlp_deep_cases.py that was).

  python -m pytest -m gpu tests/test_gpu_mlp_deep.py --junitxml=report.xml
  python profiles/tools/mlp_deep_margins.py report.xml > profiles/mlp_deep_parity_margins.txt"""
import sys
import xml.etree.ElementTree as ET


def main(path):
    rows = []
    for case in ET.parse(path).getroot().iter("testcase"):
        props = {p.get("name"): p.get("value") for p in case.iter("property")}
        if "margin" in props:
            rows.append((case.get("name"), float(props["margin"]), props.get("bar", "")))
    four = [r for r in rows if r[2] == "4-unit"]
    print("# csrc/pds_mlp_deep.hip against float64 autograd: largest ratio to the bar that applied, per case of")
    print("# tests/test_gpu_mlp_deep.py (two-layer: the bar of the two-hidden-layer kernels; 4-unit: 4 x the distance of float32 torch")
    print(f"# from float64).  {len(rows)} cases, worst {max(r[1] for r in rows):.3f}; cases that needed the 4-unit side: "
          f"{', '.join(r[0] for r in four) if four else 'none'}")
    for name, margin, bar in rows:
        print(f"{name:110s} {margin:7.3f}  {bar}")


if __name__ == "__main__":
    main(sys.argv[1])
