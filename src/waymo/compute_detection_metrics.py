#!/usr/bin/env python3
"""Native stand-in for waymo-open-dataset's compute_detection_metrics_main: reads a prediction and a ground-truth
`metrics_pb2.Objects` file and prints the 32 breakdown lines (mAP / mAPH per type and range, LEVEL_1 / LEVEL_2) in the
binary's format, so fusion.parse_waymo_metrics reads them alike.  The matching and counting run on the GPU
(cm3d_waymo_metrics); --host runs the numpy restatement instead (small files).

    python src/waymo/compute_detection_metrics.py pred.bin gt.bin [--host]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")))

from cm3d_amd import waymo_eval  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("pred", help="prediction Objects file")
    ap.add_argument("gt", help="ground-truth Objects file")
    ap.add_argument("--host", action="store_true", help="numpy restatement instead of the GPU")
    a = ap.parse_args(argv)
    for p in (a.pred, a.gt):
        if not os.path.isfile(p):
            ap.error(f"no such file: {p}")
    _, text = waymo_eval.evaluate_files(a.pred, a.gt, device=not a.host)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
