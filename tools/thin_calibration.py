"""The figures that tests/test_gpu_thin_heldout.py compares the device's ``thin.rank_curve`` with: the numpy models of THIN-1
(tests/thin_model.py) and of the glmpca loop (tests/factors_model.py, numpy's own sums, the gene half through the transposed
cell half) on matrices drawn from a log-bilinear truth of rank 3, under the Poisson law and under smoke()'s.
tests/thin_quality.py holds the protocol.  Needs no device.

    python tools/thin_calibration.py [--seeds 24] [--write]      prints the table of DESIGN section 37 and the constants of
                                                                 tests/thin_quality.py; --write puts them there
"""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import thin_quality as Q
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=24)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    peak, gain31, gain63 = {}, {}, {}
    for law, (alpha, beta) in Q.LAWS.items():
        t0 = time.time()
        curves = np.array([Q.model_curve(seed, law) for seed in range(args.seeds)])
        at = np.array(Q.KS)[np.argmax(curves, axis=1)]
        d31 = curves[:, Q.KS.index(3)] - curves[:, Q.KS.index(1)]
        d63 = curves[:, Q.KS.index(6)] - curves[:, Q.KS.index(3)]
        peak[law] = float(np.mean(at == Q.RANK))
        gain31[law] = (float(d31.mean()), float(d31.std(ddof=1)))
        gain63[law] = (float(d63.mean()), float(d63.std(ddof=1)))
        print("%s (alpha = %g, beta = %g), %d seeds (%.0f s): held-out maximum at k = 1 .. 6 in %s seeds, at the true rank in %.0f %%; "
              "Q(3) - Q(1) = %.1f (sd %.1f), Q(6) - Q(3) = %.1f (sd %.1f); mean curve minus its value at 3: %s"
              % (law, alpha, beta, args.seeds, time.time() - t0, [int((at == k).sum()) for k in Q.KS], 100.0 * peak[law],
                 *gain31[law], *gain63[law], np.round((curves - curves[:, 2:3]).mean(axis=0), 1).tolist()), flush=True)
    lines = ["SEEDS = %d" % args.seeds,
             "PEAK_AT_RANK = {%s}" % ", ".join('"%s": %.4f' % item for item in peak.items()),
             "GAIN_3_OVER_1 = {%s}" % ", ".join('"%s": (%.1f, %.1f)' % (law, *v) for law, v in gain31.items()),
             "GAIN_6_OVER_3 = {%s}" % ", ".join('"%s": (%.1f, %.1f)' % (law, *v) for law, v in gain63.items())]
    print("\n".join(lines))
    if args.write:
        path = os.path.join(ROOT, "tests", "thin_quality.py")
        text = open(path).read()
        text = re.sub(r"(---- begin\n).*?(# ---- end)", lambda m: m.group(1) + "\n".join(lines) + "\n" + m.group(2), text, flags=re.S)
        open(path, "w").write(text)


if __name__ == "__main__":
    main()
