"""Shared helpers of the Waymo metrics tests: the G11 fixtures (tests/golden/g11_waymo_metrics.json.gz, printed by the
reference's evaluator binary) and the fixture generator's synthetic sets."""
import base64
import functools
import gzip
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(None)
def fixtures():
    with open(os.path.join(HERE, "golden", "g11_waymo_metrics.json.gz"), "rb") as f:
        return json.loads(gzip.decompress(f.read()))


def blob(s):
    return base64.b64decode(s)


@functools.lru_cache(None)
def generator():
    spec = importlib.util.spec_from_file_location("gen_golden_waymo_metrics", os.path.join(HERE, "golden", "gen_golden_waymo_metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod
