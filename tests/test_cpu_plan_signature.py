"""The lowering is a pure function of the module tree, the shape, the dtype and the plan options, and it runs on CPU tensors: every plan the
package lowers must stay THE SAME plan -- launch for launch, argument for argument, region for region, with the same lane schedule.

`tests/golden/plan_signatures.json` holds, per case, the launch count and the SHA-256 of the canonical record (`tests/plan_signature.py`).
It was generated from the commit BEFORE the lowering was gathered into `_Lowering.lower()` -- from that commit's unmodified package, by
calling its `model.compile()` with a CPU tensor whose `is_cuda` answers True (a throwaway tensor subclass; that `compile()` refused CPU
tensors although it launched nothing) and `train.TrainPlan` under `train.DRY_LOWERING`.  Two separate processes gave identical digests.
The digests are never regenerated from the code under test: a lowering change that is meant to change a plan replaces the fixture from
the old code's point of view, by hand, with the reason.

The training cases after the first three (`train-v2-fp32` ... `train-canonical-bf16-protos`: another variant, BatchNorm in eval, tail
buckets, the fused switches off, four subsets of active outputs) were added the same way from commit 7dca8d6, the parent of the change
that moved the state of one backward lowering into `train._BackwardPass`: that commit's unmodified package with this helper copied
in, two separate processes, identical digests.  The 38 older entries were left byte for byte as they were.

On a mismatch: `python tests/plan_signature.py <case>` prints the full record; diff it against the same command in the other checkout."""
import json

import pytest
import torch

import plan_signature as PS

with open(PS.FIXTURE) as f:
    GOLDEN = json.load(f)


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    import os
    for k in [k for k in os.environ if k.startswith("MTBT_")]:
        monkeypatch.delenv(k)


def test_fixture_holds_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(PS.all_case_ids())
    assert len(PS.inference_cases()) == 33 + 2 and len(PS.TRAINING_CASES) == 3 + 8
    # the parent's launch counts the cases were specified with
    assert [GOLDEN[f"canonical-bf16-{k}"]["launches"] for k in ("default", "merged", "early", "trainheads")] == [193, 163, 185, 239]
    assert [GOLDEN[f"canonical-bf16-{k}-16x640"]["launches"] for k in ("default", "merged")] == [192, 162]
    assert [GOLDEN[k]["launches"] for k in PS.TRAINING_CASES] == [
        [330, 621], [335, 621], [207, 425],
        [293, 549], [335, 621], [330, 621], [336, 639],            # v2-fp32, fp32-bneval, bf16-tail, bf16-unfused
        [522], [438], [536], [399]]                                # bf16-step, -logits, -segmc, -protos: the backward plan alone


@pytest.mark.parametrize("case", list(PS.inference_cases()))
def test_inference_plan_is_the_parents_plan(case):
    assert PS.case_entry(case) == GOLDEN[case]


@pytest.mark.parametrize("case", list(PS.TRAINING_CASES))
def test_training_plans_are_the_parents_plans(case):
    assert PS.case_entry(case) == GOLDEN[case]


ACTIVE_SETS = {**PS.SUBSETS, "all": ("det", "seg", "mc", "protos", "logits")}


def test_backward_plans_do_not_depend_on_the_plans_built_before():
    """Nothing of one backward lowering outlives it: on ONE `TrainPlan` the plans for four subsets of the outputs and then for all five
    are each the plan a fresh `TrainPlan` lowers first (the fixture's entries, which come from a fresh plan per case)."""
    model, tp = PS.lower_training("train-canonical-bf16")
    for k, active in ACTIVE_SETS.items():
        rec = PS.training_plan_record(model, tp, active)
        want = GOLDEN["train-canonical-bf16" + ("" if k == "all" else "-" + k)]
        assert (len(rec["launches"]), PS.digest(rec)) == (want["launches"][-1], want["sha256"][-1]), k


def test_backward_plan_is_built_once_per_set_of_outputs():
    _, tp = PS.lower_training("train-canonical-bf16")
    with PS.dry_lowering():
        plan = tp.backward_plan(("det", "logits", "protos"))
        assert tp.backward_plan(("protos", "det", "logits")) is plan and tp.backward_plan(["logits", "protos", "det"]) is plan
        assert tp.backward_plan(("logits",)) is not plan


@pytest.mark.parametrize("variant,fewer", [("canonical", 30), ("v2", 6)])
def test_merged_plan_launch_counts_on_cpu(variant, fewer):
    """tests/test_gpu_conv_batch.py::test_merged_plan_launch_counts without a device: 19 -> 9 launches per level (v2, Segment alone:
    11 -> 9); a head BatchNorm in training mode keeps the separate lowering completely."""
    model = PS.make_model(variant, "fp32")

    def names(opt):
        model.plan_options = {"HEADS_MERGED": opt}
        return [l.name for l in PS.lower_inference(model, (2, 3, 256, 256)).plan.launches]
    sep, mer = names("0"), names("1")
    assert len(sep) - len(mer) == fewer
    batches = [n for n in mer if " + " in n]
    assert len(batches) == (8 if fewer == 30 else 2) * 3
    model.segment.cv4[1][0].bn.train()
    sep_t, mer_t = names("0"), names("1")
    assert len(sep_t) - len(mer_t) == fewer * 2 // 3          # level 1 falls back, the other two stay merged
    for m in model.segment.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.train()
    assert names("0") == names("1")


def test_weights_signature_follows_module_surgery():
    """`_weights_sig` pairs the BatchNorm modules of THIS call's walk with their modes: a replaced BatchNorm changes the signature (a list
    cached at the first call would still hold the old module), and a modes tuple of another length is an error, never a truncation."""
    model = PS.make_model("canonical", "fp32")
    before = model._weights_sig()
    assert model._weights_sig() == before and model._weights_sig(model._bn_modes()) == before
    old = model.neck.p3_proj.bn
    new = torch.nn.BatchNorm2d(old.num_features, momentum=old.momentum, eps=old.eps).eval()
    with torch.no_grad():
        new.weight.copy_(old.weight)
        new.bias.copy_(old.bias)
        new.running_mean.fill_(0.25)
        new.running_var.fill_(2.0)
    # parameters in place (same storage, same version): only the running statistics tell the two modules apart
    new.weight, new.bias = old.weight, old.bias
    model.neck.p3_proj.bn = new
    assert model._weights_sig() != before
    modes = model._bn_modes()
    with pytest.raises(ValueError):
        model._weights_sig(modes[:-1])
    with pytest.raises(ValueError):
        model._weights_sig(modes + (False,))
