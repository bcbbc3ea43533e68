"""The reference program's own known answers for pair_style soft, as data: energy, forces and stress of data.fourmol.

  unittest/force-styles/tests/mol-pair-soft.yaml            -> pair_soft.json

Beside make_golden.py, whose parser and reference location it uses; fourmol.json (the system) is make_golden.py's.

    python tests/golden/make_soft_golden.py [reference_dir]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else mg.REF
    g = mg.known_answers(os.path.join(ref, "unittest", "force-styles", "tests", "mol-pair-soft.yaml"), "vdwl")
    # pair_style soft 8.0, post_commands: pair_modify mix arithmetic (values of the harness the answers were made with)
    g.update({"pair_style": "soft", "cut_global": 8.0, "mix": "arithmetic"})
    json.dump(g, open(os.path.join(mg.OUT, "pair_soft.json"), "w"))
    print("pair_soft.json: %d forces, epsilon %g" % (len(g["init_forces"]), g["epsilon"]))


if __name__ == "__main__":
    main()
