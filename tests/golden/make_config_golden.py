#!/usr/bin/env python3
"""Generate tests/golden/configs_merged.json by running the REFERENCE's load_config (build container only).

    python tests/golden/make_config_golden.py

Like make_golden.py it imports the reference in place and stores results only: the merged config dict of the three leaf
files, as the reference's own src/config.py:load_config returns them when run from the reference's root (its
`inherit_from` paths are relative to that directory) with configs/ESLAM.yaml as the default, which is how run.py calls
it.  The YAML files under tests/golden/configs/ are copies of the reference's settings files.
"""
import importlib
import json
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "configs_merged.json")
LEAVES = ("Replica/room0.yaml", "ScanNet/scene0000.yaml", "TUM_RGBD/freiburg1_desk.yaml")
sys.dont_write_bytecode = True


def main():
    # src/config.py imports src.networks for its model factory only: an empty stand-in, the package itself in place
    pkg = types.ModuleType("src")
    pkg.__path__ = [os.path.join(REF, "src")]
    sys.modules["src"] = pkg
    sys.modules["src.networks"] = types.ModuleType("src.networks")
    ref_config = importlib.import_module("src.config")
    os.chdir(REF)
    merged = {leaf: ref_config.load_config(os.path.join("configs", leaf), "configs/ESLAM.yaml") for leaf in LEAVES}
    with open(OUT, "w") as f:
        json.dump(merged, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
