"""echoseal_amd.pipeline imports echoseal_amd.engine, and engine hands out the pipeline's public names: whichever of the two a fresh
interpreter imports first, both load and both name the same objects.  Importing needs no GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("DecodePipeline", "GroupTicket", "hw_queue_budget", "pipeline_streams")


@pytest.mark.parametrize("first, second", [("engine", "pipeline"), ("pipeline", "engine")])
def test_either_module_first(first, second):
    code = (f"import echoseal_amd.{first} as a\nimport echoseal_amd.{second} as b\n"
            f"from echoseal_amd.engine import DecodePipeline, GroupTicket, RxEngine, hw_queue_budget, pipeline_streams\n"
            f"assert all(getattr(a, n) is getattr(b, n) for n in {NAMES!r})\n"
            f"assert DecodePipeline is a.DecodePipeline and callable(DecodePipeline) and hw_queue_budget() >= 1\n"
            f"print('same objects')\n")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "same objects", p.stderr
