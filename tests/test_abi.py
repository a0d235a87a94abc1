"""CPU: the C-ABI library loads without a GPU, exports exactly what include/mbrl_cem.h declares,
and the ctypes structs match the C layout (checked against gcc on the header itself)."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "mbrl_cem.h")


def declared_functions():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mbrl_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from mbrl_amd import _lib
    lib = _lib.load()
    decl = declared_functions()
    assert decl == sorted(_lib.EXPORTED)
    for name in decl:
        assert hasattr(lib, name), name
    assert lib.mbrl_abi_version() == _lib.ABI_VERSION == 13


def test_no_gpu_needed_for_sizing_calls():
    from mbrl_amd import _lib
    lib = _lib.load()
    sh = _lib.MlpShape(17, 6, 512, 3, 1)
    # 68 chunks x 8 KiB per wave x 4 waves + biases (3*512 + 32) + plain copies for the trajectory
    # kernel (W^T of layer 0 and the two hidden layers, row-major output layer), 64-float aligned
    plain = 23 * 512 + 2 * 512 * 512 + 17 * 512
    # then the split streams: 34 chunks of 32 K rows (1 + 2 x 16 + 1) x 8 waves x 8 KiB (F16X3: two
    # pieces) or x 12 KiB (F16X6: three pieces), each followed by a flag word
    a64 = lambda x: (x + 63) // 64 * 64   # noqa: E731
    split = 34 * 2048 * 8 + 64 + 34 * 3072 * 8 + 64
    # then the 8-candidate stream: 2 + 2 x 32 + 2 chunks of 16 K rows x 8 waves x 4 KiB
    m8 = 68 * 8192
    # then the 4-candidate stream: 2 + 2 x 32 layer-0 / hidden chunks + 4 output chunks x 8 waves x 4 KiB
    m4 = 70 * 8192
    assert lib.mbrl_mlp_packed_bytes(ctypes.byref(sh)) == \
        a64(a64(68 * 8192 + 3 * 512 + 32 + plain) + split + m8) * 4 + m4 * 4
    # precision does not change the packed layout; an unknown precision is rejected
    assert lib.mbrl_mlp_packed_bytes(ctypes.byref(_lib.MlpShape(17, 6, 512, 3, 1, 0, 1))) == \
        lib.mbrl_mlp_packed_bytes(ctypes.byref(sh))
    assert lib.mbrl_mlp_packed_bytes(ctypes.byref(_lib.MlpShape(17, 6, 512, 3, 1, 0, 2))) == \
        lib.mbrl_mlp_packed_bytes(ctypes.byref(sh))
    assert lib.mbrl_mlp_packed_bytes(ctypes.byref(_lib.MlpShape(17, 6, 512, 3, 1, 0, 7))) == 0
    bad = _lib.MlpShape(17, 6, 4096, 3, 1)
    assert lib.mbrl_mlp_packed_bytes(ctypes.byref(bad)) == 0
    assert lib.mbrl_select_workspace_bytes(4096) >= 4096 * 4
    assert lib.mbrl_refit_workspace_bytes(30, 6, 409) >= 30 * 6 * 409 * 4
    p = _lib.CemParams(4096, 30, 409, 5, 0.1, -1.0, 1.0, 0.0, 0.5, 0, 1)
    assert lib.mbrl_cem_workspace_bytes(ctypes.byref(sh), ctypes.byref(p)) > 4096 * 4
    # reward head: one more output row (17 + 1 still fits two 16-row tiles) and its plain copy
    shr = _lib.MlpShape(17, 6, 512, 2, 1, 1)
    plain_r = 23 * 512 + 512 * 512 + 18 * 512
    split_r = 18 * 2048 * 8 + 64 + 18 * 3072 * 8 + 64
    assert lib.mbrl_mlp_packed_bytes(ctypes.byref(shr)) == a64(a64(36 * 8192 + 2 * 512 + 32 + plain_r) + split_r) * 4
    assert lib.mbrl_mlp_packed_bytes(ctypes.byref(_lib.MlpShape(17, 6, 512, 2, 1, 2))) == 0


def test_errors_are_reported_not_crashing():
    from mbrl_amd import _lib
    lib = _lib.load()
    sh = _lib.MlpShape(0, 6, 512, 3, 1)
    rc = lib.mbrl_mlp_pack(ctypes.byref(sh), None, None, None, None)
    assert rc == -2
    assert b"unsupported MLP shape" in lib.mbrl_last_error()
    rc = lib.mbrl_select_elites(None, 1, 10, 20, 0, None, None, None, 0, None)
    assert rc == -1
    # mbrl_gd_grad refuses before anything touches a GPU: a NULL grad_out, then mbrl_gd_plan_batch's checks
    good = _lib.MlpShape(17, 6, 512, 3, 1)
    cost = _lib.Cost(_lib.MBRL_COST_GOAL_STATE, 1, 1, 0, None, None, 0.4, 0.25)
    one = ctypes.c_void_p(16)      # a non-NULL pointer nobody dereferences on these paths
    assert lib.mbrl_gd_grad(ctypes.byref(good), one, None, ctypes.byref(cost), one, one, 1, 4, None, one, one, 0,
                            None) == _lib.MBRL_EINVAL
    assert b"grad_out" in lib.mbrl_last_error()
    assert lib.mbrl_gd_grad(ctypes.byref(sh), one, None, ctypes.byref(cost), one, one, 1, 4, one, one, one, 0,
                            None) == _lib.MBRL_EUNSUPPORTED
    assert lib.mbrl_gd_grad(ctypes.byref(good), one, None, None, one, one, 1, 4, one, one, one, 0,
                            None) == _lib.MBRL_EUNSUPPORTED
    assert lib.mbrl_gd_grad(ctypes.byref(good), one, None, ctypes.byref(cost), one, one, 1, 4, one, None, one, 0,
                            None) == _lib.MBRL_EINVAL
    assert lib.mbrl_gd_grad(ctypes.byref(good), one, None, ctypes.byref(cost), one, one, 0, 4, one, one, one, 0,
                            None) == _lib.MBRL_EINVAL
    # (state cost without weights / goal)
    assert lib.mbrl_gd_grad(ctypes.byref(good), one, None, ctypes.byref(cost), one, one, 1, 4, one, one, one, 0,
                            None) == _lib.MBRL_EINVAL
    cost.has_state_cost = 0
    assert lib.mbrl_gd_grad(ctypes.byref(good), one, None, ctypes.byref(cost), one, one, 1, 4, one, one, one, 0,
                            None) == _lib.MBRL_EWORKSPACE


def test_gd_entries_take_the_arguments_the_header_declares():
    """The ctypes signature table against include/mbrl_cem.h for the gradient-descent entries: as many
    arguments, integers and floats where the header has them, pointers elsewhere."""
    from mbrl_amd import _lib
    lib = _lib.load()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    kinds = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    for name in ("mbrl_gd_grad", "mbrl_gd_plan", "mbrl_gd_plan_batch"):
        params = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")
        want = []
        for prm in params:
            words = prm.replace("*", " * ").split()
            want.append("ptr" if "*" in words or "mbrl_stream_t" in words else kinds[words[-2]])
        fn = getattr(lib, name)
        got = ["ptr" if t is ctypes.c_void_p or hasattr(t, "contents") else t for t in fn.argtypes]
        assert got == want, name
        assert fn.restype is ctypes.c_int32
    assert len(lib.mbrl_gd_grad.argtypes) == 13


STRUCTS = {
    "MlpShape": ("mbrl_mlp_shape", ["state_dim", "action_dim", "hidden", "n_hidden", "ensemble", "reward_head",
                                    "precision"]),
    "Norm": ("mbrl_norm", ["obs_mean", "obs_std", "act_mean", "act_std", "rew_mean", "rew_std", "normalize_state",
                           "unnormalize_state", "normalize_action", "unnormalize_reward"]),
    "Cost": ("mbrl_cost", ["kind", "has_state_cost", "has_action_cost", "weights", "goal", "alpha_state",
                           "alpha_action"]),
    "Sampler": ("mbrl_sampler", ["seed", "iteration", "mu", "sigma", "lo", "hi"]),
    "CemParams": ("mbrl_cem_params", ["N", "H", "K", "iterations", "alpha", "lo", "hi", "init_mu", "init_sigma",
                                      "seed"]),
    "AdamTensor": ("mbrl_adam_tensor", ["param", "grad", "exp_avg", "exp_avg_sq", "numel", "step_size", "bc2_sqrt"]),
    "AdamHparams": ("mbrl_adam_hparams", ["lerp_weight", "beta2", "one_minus_beta2", "eps", "weight_decay"]),
    "TrainModel": ("mbrl_train_model", ["state_dim", "action_dim", "hidden", "n_hidden", "reward_head", "horizon",
                                        "weight", "bias", "weight_grad", "bias_grad"]),
    "TrainData": ("mbrl_train_data", ["states", "actions", "next_states", "rewards", "transitions"]),
}


def test_ctypes_layout_matches_c_header():
    from mbrl_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for py, (c, fields) in STRUCTS.items():
        lines.append(f'printf("{py} sizeof %zu\\n", sizeof({c}));')
        for f in fields:
            lines.append(f'printf("{py} {f} %zu\\n", offsetof({c}, {f}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        try:
            subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True, capture_output=True)
        except (FileNotFoundError, subprocess.CalledProcessError) as e:  # pragma: no cover
            pytest.skip(f"gcc unavailable: {e}")
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    for line in filter(None, out):
        py, field, val = line.split()
        cls = getattr(_lib, py)
        if field == "sizeof":
            assert ctypes.sizeof(cls) == int(val), py
        else:
            assert getattr(cls, field).offset == int(val), (py, field)


def test_library_resolves_every_symbol_at_load():
    """RTLD_NOW: an internal symbol left undefined (a definition in the wrong namespace, say) fails
    here instead of at the first call on a GPU box."""
    import os
    from mbrl_amd import _lib
    ctypes.CDLL(_lib.LIB_PATH, mode=os.RTLD_NOW)


def test_single_gpu_library_does_not_link_rccl():
    """RCCL is opened on the first mbrl_comm_* / sharded call (dlopen), so the library's
    dynamic section names no librccl and single-GPU use loads without it."""
    from mbrl_amd import _lib
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    # DT_NEEDED entries are strings in .dynstr; the dlopen target appears only as a string literal,
    # so check the dynamic section's NEEDED list through the ELF reader
    import subprocess
    out = subprocess.run(["readelf", "-d", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = [ln for ln in out.splitlines() if "(NEEDED)" in ln]
    assert needed and not any("rccl" in ln for ln in needed), needed
    assert b"librccl.so.1" in blob   # the run-time dlopen target


def test_split_stream_bytes_match_the_packed_geometry():
    """bench.py's L2 roofline for the split kernels uses synthetic.split_stream_bytes_per_step; it must
    equal the stream the pack writes (the packed-size test above: 34 chunks for cheetah)."""
    from mbrl_amd import synthetic
    ch = synthetic.CONFIGS[3]
    assert synthetic.split_stream_bytes_per_step(ch, 2) == 34 * 2048 * 8 * 4
    assert synthetic.split_stream_bytes_per_step(ch, 3) == 34 * 3072 * 8 * 4
    rw = dict(ch, L=2, reward=True)
    assert synthetic.split_stream_bytes_per_step(rw, 2) == 18 * 2048 * 8 * 4


def test_options_are_set_through_the_abi_not_the_environment():
    """mbrl_set_option / mbrl_get_option (MBRL_OPT_*): set, restore, reject unknown options and
    values; no source of the library reads the environment (a stray variable cannot redirect a
    production launch)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    for name, code in _lib.OPTIONS.items():
        assert lib.mbrl_get_option(code) == 0, name
    with _lib.option("rollout_tile", 8):
        assert lib.mbrl_get_option(_lib.OPTIONS["rollout_tile"]) == 8
        with _lib.option("rollout_tile", 16):
            assert lib.mbrl_get_option(_lib.OPTIONS["rollout_tile"]) == 16
        assert lib.mbrl_get_option(_lib.OPTIONS["rollout_tile"]) == 8
    assert lib.mbrl_get_option(_lib.OPTIONS["rollout_tile"]) == 0
    assert lib.mbrl_set_option(_lib.OPTIONS["rollout_tile"], 12) < 0
    assert lib.mbrl_get_option(_lib.OPTIONS["rollout_tile"]) == 0
    assert lib.mbrl_set_option(99, 1) < 0 and lib.mbrl_get_option(99) < 0
    with pytest.raises(RuntimeError):
        with _lib.option("gd_single", 5):
            pass
    csrc = os.path.join(REPO, "mujoco-mbrl_amd", "csrc")
    for f in os.listdir(csrc):
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f


def test_training_workspace_and_status_word_sizing():
    """mbrl_train_workspace_bytes / mbrl_train_status_offset need no GPU: the fused step's status word
    lies inside the workspace, 4-byte aligned, for every shape; bad shapes give 0 / (size_t)-1."""
    from mbrl_amd import _lib
    lib = _lib.load()
    for s, a, W, L, reward, H, B in [(17, 6, 512, 2, 0, 1, 512), (17, 6, 200, 2, 1, 1, 400), (5, 1, 50, 3, 0, 2, 37)]:
        m = _lib.TrainModel()
        m.state_dim, m.action_dim, m.hidden, m.n_hidden, m.reward_head, m.horizon = s, a, W, L, reward, H
        need = lib.mbrl_train_workspace_bytes(ctypes.byref(m), B)
        at = lib.mbrl_train_status_offset(ctypes.byref(m), B)
        assert need > 0 and at % 4 == 0 and at + 4 <= need, (s, W, L, need, at)
    bad = _lib.TrainModel()
    bad.state_dim, bad.action_dim, bad.hidden, bad.n_hidden, bad.reward_head, bad.horizon = 17, 6, 512, 0, 0, 1
    assert lib.mbrl_train_workspace_bytes(ctypes.byref(bad), 512) == 0
    assert lib.mbrl_train_status_offset(ctypes.byref(bad), 512) == ctypes.c_size_t(-1).value


def test_library_was_built_from_this_tree():
    """mbrl_build_info() carries the sha256 prefix of the sources the .so was compiled from
    (mujoco-mbrl_amd/Makefile DIGEST_FILES); it must equal the digest of the sources in this tree,
    so a prebuilt library that travels with the tree is known to be these sources' build."""
    from mbrl_amd import _lib
    built, same = _lib.build_info()
    assert same, f"libmbrl_cem.so was built from sources {built}, the tree holds {_lib.source_digest()}: rebuild"


def test_shard_options_and_peer_status_code():
    """ABI v13: MBRL_OPT_SHARD_EMULATE takes 0 / 1 / 2 (2: the per-rank timing mode) and
    MBRL_OPT_DEBUG_SHARD_FAIL_RANK names the failing rank; MBRL_EPEER is -5 in the header and here."""
    from mbrl_amd import _lib
    lib = _lib.load()
    code = _lib.OPTIONS["shard_emulate"]
    for v in (1, 2):
        with _lib.option("shard_emulate", v):
            assert lib.mbrl_get_option(code) == v
    assert lib.mbrl_set_option(code, 3) < 0 and lib.mbrl_get_option(code) == 0
    with _lib.option("debug_shard_fail_rank", 4):
        assert lib.mbrl_get_option(_lib.OPTIONS["debug_shard_fail_rank"]) == 4
    hdr = open(os.path.join(REPO, "include", "mbrl_cem.h")).read()
    assert "MBRL_EPEER = -5" in hdr and _lib.MBRL_EPEER == -5
    assert "MBRL_OPT_DEBUG_SHARD_FAIL_RANK = 20" in hdr and "MBRL_OPT_COUNT = 22" in hdr


def test_every_compile_time_variant_still_compiles():
    """The kept compile-time variants (stamp builds and the rollout's timing ablations, Makefile
    `variants`) compile against the current sources, so none of them rots unseen."""
    import shutil
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", os.path.join(REPO, "mujoco-mbrl_amd"), "variants"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " error" not in r.stderr, r.stderr[-2000:]
