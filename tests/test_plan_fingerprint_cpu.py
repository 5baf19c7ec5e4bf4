"""The recorded plans of every engine (UNet, LGM, VAE, CLIP towers) are pinned launch by launch: tools/plan_fingerprint.py records the
production plans on the CPU (zero weights, the real library's host-side answers) and hashes every field of every recorded parameter
block with the pointers made address-independent.  tests/golden/plan_fingerprints.json holds the fingerprints of the commit before the
engines moved onto plan_builder.PlanBuilder: equal fingerprints = the same launches, in the same order, with the same parameters and
the same buffer reuse.  A change that is MEANT to alter a plan regenerates the file (tools/plan_fingerprint.py --out) and says so."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    from videomv_amd import _lib as L
    with open(os.path.join(golden_dir, "plan_fingerprints.json")) as f:
        return json.load(f)[L.elem_name()]


@pytest.fixture(scope="module")
def recorded():
    spec = importlib.util.spec_from_file_location("plan_fingerprint", os.path.join(ROOT, "tools", "plan_fingerprint.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.fingerprints()


def test_the_matrix_is_the_pinned_one(golden, recorded):
    assert set(recorded) == set(golden), sorted(set(recorded) ^ set(golden))


def test_recorded_plans_equal_the_pinned_fingerprints(golden, recorded):
    differ = [f"{name}: ops {fp['ops']} (pinned {golden[name]['ops']}), per op code {fp['by_op']} (pinned {golden[name]['by_op']})"
              for name, fp in recorded.items() if fp != golden.get(name)]
    assert not differ, ("recorded plans differ from the pinned ones (python tools/plan_fingerprint.py --dump DIR on both trees, then diff):\n"
                        + "\n".join(differ))


def test_pinned_fingerprints_are_those_of_the_production_plans(golden):
    # recording the plan again gives the fresh engine's plan; a switch that does not apply to a network leaves its plan alone
    assert golden["unet.tiny.rerecord"] == golden["unet.tiny"] == golden["unet.tiny.tqa0"]
    assert golden["unet.tiny.taps"]["ops"] == golden["unet.tiny"]["ops"] and golden["unet.tiny.taps"] != golden["unet.tiny"]
    assert golden["unet.full.B2.24x40x64.shared"]["ops"] == {"S": 766, "Sctx": 16}
    assert golden["lgm.big.256.batch1"]["ops"] == golden["lgm.big.256.batch2"]["ops"] == {"S": 218}
    assert golden["vae.decoder.n8.40x64"]["ops"] == {"S": 101} and golden["vae.encoder.n4.256x256"]["ops"] == {"S": 67}
    assert golden["clip.text.B2.donor"]["ops"] == {"S": 162} and golden["clip.vision.B1"]["ops"] == {"S": 225}
