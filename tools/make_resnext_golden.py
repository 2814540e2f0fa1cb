"""Record tests/golden/resnext_contract.json from the UNMODIFIED reference (needs the reference tree; oracle/refshim.py).

The reference ``ResNet`` of SLOW_8x8_R50 with RESNET.NUM_GROUPS 8 / WIDTH_PER_GROUP 4 (tests/gconv_checks.py: MODEL_OPTS) is built
through oracle.refshim, loaded with the seeded state the tests draw again, and run once in train mode (forward, cross entropy,
backward).  Recorded: the state_dict key / shape list, logits, loss, gradient norm, per-parameter gradient norms, running-statistic
sums and the torch version.  Results only: every input is a seed.

    python tools/make_resnext_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import gconv_checks as gc  # noqa: E402


def main():
    rec = gc.reference_record()
    path = os.path.join(ROOT, "tests", "golden", gc.CONTRACT + ".json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("%s: %d state entries, loss %.6f, grad_norm %.6f" % (path, len(rec["state_dict"]), rec["loss"], rec["grad_norm"]))


if __name__ == "__main__":
    main()
