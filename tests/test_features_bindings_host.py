"""mcgmil.features' bindings against a recording made before they were last rewritten
(tests/fixtures/features_bindings.json, from the commit named in it; the recorder and the cases are
tests/fixtures/make_features_bindings.py). No device and no library: the wrappers run on CPU
tensors that say they are CUDA ones, against a stub that records every call and writes a constant
of the field's own through every output pointer. What must hold: the same entry points in the same
order with the same struct fields, the same pointers NULL, the same input behind each pointer, every
returned tensor the one its output field was written through, every predicate's verdict and reason,
and every op's schema, character for character."""
import importlib.util
import json
import os

import pytest

from mcgmil import features, library  # noqa: F401

_HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures")
_spec = importlib.util.spec_from_file_location("make_features_bindings", os.path.join(_HERE, "make_features_bindings.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(rec.FIXTURE) as _fh:
    WANT = json.load(_fh)

# which output field each returned tensor must have been written through, by the wrapper's name
# (the case's name up to the first "/"); None: no tensor
RETURNS = {
    "packed_conv_weight": ["packed"], "packed_conv_weight_f32": ["packed"], "packed_stem_weight": ["packed"],
    "conv2d": ["y"], "conv2d_f32": ["y"], "conv2d_bf16": ["y"], "stem": ["y"],
    "conv2d_f32_wgrad": ["dw"], "conv2d_f32_stem_wgrad": ["dw"], "conv2d_bf16_wgrad": ["dw"],
    "conv2d_f32_dgrad_direct": ["dx"], "conv2d_f32_dgrad": ["y"], "conv2d_bf16_dgrad": ["y"],   # the forward kernel's y
    "batchnorm_act": ["y"], "batchnorm_coefficients": ["ab"],
    "batchnorm_act_stats": ["y", "batch_mean", "batch_invstd"],
    "batchnorm_pool_stats": ["y", "batch_mean", "batch_invstd", "argmax"],
    "batchnorm_act_backward": ["dx", "dresidual", "dgamma", "dbeta"],
    "batchnorm_pool_backward": ["dz", "dgamma", "dbeta"],
}


@pytest.fixture(scope="module")
def got():
    return rec.record()


def test_the_fixture_names_its_commit_and_is_small():
    assert len(WANT["generated_from"]["commit"]) == 40
    assert os.path.getsize(rec.FIXTURE) < 200_000


def test_every_case_is_in_the_fixture(got):
    assert sorted(got["wrappers"]) == sorted(WANT["wrappers"])
    for table in ("conv", "bn", "bn_pool", "stem"):
        assert sorted(got["predicates"][table]) == sorted(WANT["predicates"][table]), table


@pytest.mark.parametrize("name", sorted(WANT["wrappers"]))
def test_wrapper_calls(got, name):
    have, want = got["wrappers"][name], WANT["wrappers"][name]
    assert [c["fn"] for c in have["calls"]] == [c["fn"] for c in want["calls"]]
    for h, w in zip(have["calls"], want["calls"]):
        assert h == w, h["fn"]
    assert have["returns"] == want["returns"]


@pytest.mark.parametrize("name", sorted(WANT["wrappers"]))
def test_returned_tensors_come_from_their_fields(got, name):
    wrapper = name.split("/")[0].split("@")[0]
    returns = got["wrappers"][name]["returns"]
    if wrapper == "conv_input_bn":
        return
    want = RETURNS[wrapper]
    if wrapper in ("conv2d", "conv2d_f32") and len(returns) == 2:             # stats=True
        want = ["y", "stats"]
    if wrapper == "packed_conv_weight" and len(returns) == 2:                  # the cached call
        want = ["packed", "packed"]
    assert len(returns) == len(want)
    assert "?" not in returns
    for field, expect in zip(returns, want):
        assert field in (expect, None), (returns, want)                        # None: not asked for
    launches = [c for c in got["wrappers"][name]["calls"] if "stream" in c]
    assert all(c["stream"] is True and "unexpected_args" not in c for c in launches)
    assert any(r is not None for r in returns) == bool(launches)


@pytest.mark.parametrize("table", ["conv", "bn", "bn_pool", "stem"])
def test_predicates(got, table):
    have, want = got["predicates"], WANT["predicates"]
    said = lambda doc, v: doc["reasons"][v] if isinstance(v, int) and not isinstance(v, bool) else v  # noqa: E731
    for key, row in want[table].items():
        h = have[table][key]
        if isinstance(row, list):
            assert [said(have, v) for v in h] == [said(want, v) for v in row], key
        else:
            assert said(have, h) == said(want, row), key
    assert sorted(have["reasons"]) == sorted(want["reasons"])


def test_schemas(got):
    assert got["schemas"] == WANT["schemas"]
    assert sorted(got["schemas"]) == sorted(library.__all__)
