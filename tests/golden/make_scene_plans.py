#!/usr/bin/env python3
"""Record the kernel plan of every shipped configuration as an upload reports it (needs a GPU):
Context.scene_info() of C1-C5 and X1-X16, default host builder, BLING_BRUTE unset.  tests/test_scene_plan.py
holds the device-free bling_debug_scene_plan to these.

  python tests/golden/make_scene_plans.py      # rewrites tests/golden/scene_plans.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from bling_amd.render import Context  # noqa: E402
from bling_amd.scene import CONFIGS, FEATURE_SCENES, load_config  # noqa: E402

assert "BLING_BRUTE" not in os.environ
ctx = Context(0)
plans = {}
for name in list(CONFIGS) + list(FEATURE_SCENES):
    ctx.upload(load_config(name))
    plans[name] = ctx.scene_info()
with open(os.path.join(HERE, "scene_plans.json"), "w") as f:
    json.dump(plans, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(plans)} plans recorded")
