"""CPU: the table of tests/workspace_cases.py covers every exported function of include/mbrl_cem.h whose
prototype takes a `void* workspace` (so a new entry point cannot be added without a case), and each of its
shapes reaches the kernels it is meant to reach, by the restatement of tests/rollout_dispatch_model.py."""
import os
import re

import rollout_dispatch_model as rdm
import workspace_cases as wc

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "mbrl_cem.h")


def workspace_entries(text):
    """Names of the prototypes with a `workspace` parameter, comments stripped first."""
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = []
    for m in re.finditer(r"\b(?:int|size_t)\s+(mbrl_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*workspace\b", m.group(2)):
            names.append(m.group(1))
    return names


def test_every_entry_with_a_workspace_has_a_case():
    with open(HEADER) as f:
        names = workspace_entries(f.read())
    # the parse found what it should: the three small calls, a plan of each family, gd, training
    for known in ("mbrl_select_elites", "mbrl_cem_refit", "mbrl_trajectory", "mbrl_cem_plan", "mbrl_cem_plan_rh_batch_mixed",
                  "mbrl_mppi_update_elite", "mbrl_mppi_plan_elite_batch", "mbrl_gd_grad", "mbrl_train_epoch_ensemble"):
        assert known in names, known
    assert len(names) == len(set(names)) >= 23
    covered = wc.entries_covered()
    missing = [n for n in names if n not in covered]
    assert not missing, f"no case in tests/workspace_cases.py for: {missing}"
    assert covered <= set(names), covered - set(names)          # a case names only real entries


def test_the_parse_sees_a_new_entry():
    proto = "int mbrl_new_plan(const float* s0, float* out, void* workspace,\n    size_t ws_bytes, mbrl_stream_t stream);"
    assert workspace_entries("/* void* workspace in a comment (x); */ size_t mbrl_q(int N);\n" + proto) == ["mbrl_new_plan"]


def test_single_model_training_is_the_only_zeroed_exception():
    once = {e for c in wc.CASES.values() if c.zeroed_once for e in c.entries}
    assert once == {"mbrl_train_grads", "mbrl_train_epoch"}
    assert not once & {e for c in wc.CASES.values() if not c.zeroed_once for e in c.entries}


def test_shapes_reach_the_kernels_they_are_meant_to():
    for shape, want in wc.TRAJECTORY.items():
        sh = wc.SHAPES[shape]
        o = sh["over"]
        assert rdm.trajectory_kernel(o["s"], o["a"], o["W"], o["L"], o["E"], H=sh["H"]) == want, shape
        inst = rdm.dispatch(o["s"], o["a"], o["W"], o["L"], o["E"], N=sh["N"])
        assert isinstance(inst, rdm.Instance), (shape, inst)       # the rollout is not refused
        g = rdm.geometry(o["s"], o["a"], o["W"], o["L"], o["E"])
        # plan.hip pair_area_bytes: a pair area only at Wpad = 512 with at most 256 pair workgroups
        pairs = g["T"] == 8 and 2 * ((sh["N"] + 15) // 16) * o["E"] <= 256
        assert pairs == (shape in ("pair", "wide")), shape
    p = wc.SHAPES["pair"]
    assert (p["N"] + 15) // 16 == 2 and p["N"] % 16                 # two tiles, the second one ragged
    assert p["over"]["s"] > 16 and p["over"]["s"] % 16               # a padded output chunk
    e = wc.SHAPES["ens"]["over"]
    assert e["E"] == 3 and e["W"] == 64
    assert wc.SHAPES["plain"]["over"]["s"] > 80
    # gd.hip gd_coop_supported's static half: the cooperative kernel takes W 64, L 2, s + a <= 32
    g = wc.GD["over"]
    assert g["W"] in (64, 128, 256, 512) and g["L"] >= 2 and g["s"] + g["a"] <= 32 and wc.GD["H"] == 3
    # fused_step (csrc/train.hip): the fused three-launch step at two hidden layers, batch x horizon rows
    assert wc.TRAIN["batch"] * wc.TRAIN["horizon"] == 260 and wc.TRAIN_ROWS % wc.TRAIN["batch"]


def test_every_plan_runs_fused_and_unfused():
    plans = [n for n in wc.CASES if "_plan" in n and not n.startswith("gd_") and "update_split" not in n]
    for n in plans:
        if not n.endswith("_unfused"):
            assert n + "_unfused" in wc.CASES, n
