"""CPU: the byte counts of the six workspace queries, frozen. Every query is host arithmetic (no GPU):
a carver lays its buffers out in a fixed order, each rounded up to 256 bytes, so the total pins both
the order-independent sizes and every branch that adds or drops a buffer (the column-split pair
area, the MPPI plan's second proposal buffer, the sharded plan's emulation buffers). A carver that
is reordered, realigned or loses a buffer changes one of these numbers."""
import ctypes

import pytest

# name -> (state_dim, action_dim, hidden, n_hidden, ensemble), (N, H, K)
SHAPES = {
    "cartpole": ((4, 1, 64, 2, 1), (1024, 20, 102)),       # narrow model, no pair area
    "cheetah": ((17, 6, 512, 3, 1), (4096, 30, 409)),      # 512 workgroups > 256: no pair area
    "cheetah_n1024": ((17, 6, 512, 3, 1), (1024, 30, 102)),   # pair area present
    "humanoid": ((67, 21, 512, 3, 5), (32768, 50, 3276)),  # ensemble
}

# The literal bytes the library returned before the carvers shared a helper.
EXPECTED = {
    "cartpole": {"traj": 1792, "cem": 102656, "mppi": 171008, "shard1": 110848, "shard8": 35584,
                 "shard8_emu": 66304, "batch16": 1723904, "gd1": 12800, "gd16": 200960},
    "cheetah": {"traj": 10496, "cem": 3293952, "mppi": 5928448, "shard1": 3326720, "shard8": 3427328,
                "shard8_emu": 3877888, "batch16": 52275712, "gd1": 197376, "gd16": 3154176},
    "cheetah_n1024": {"traj": 10496, "cem": 6224640, "mppi": 6883072, "shard1": 6232832, "shard8": 867584,
                      "shard8_emu": 980224, "batch16": 13111296, "gd1": 197376, "gd16": 3154176},
    "humanoid": {"traj": 108288, "cem": 152324096, "mppi": 138407168, "shard1": 153634816, "shard8": 32638976,
                 "shard8_emu": 53118976, "batch16": 2355898624, "gd1": 342016, "gd16": 5468416},
}


def _queries(lib, _lib, name):
    shape, (N, H, K) = SHAPES[name]
    sh = _lib.MlpShape(*shape)
    p = _lib.CemParams(N, H, K, 5, 0.1, -1.0, 1.0, 0.0, 0.5, 0, 1)
    mp = _lib.MppiParams(N, H, 5, 0, 1.0, 0.1, -1.0, 1.0, 0.0, 0.5, 1)
    r, rp, rm = ctypes.byref(sh), ctypes.byref(p), ctypes.byref(mp)
    out = {
        "traj": lib.mbrl_trajectory_workspace_bytes(r, H),
        "cem": lib.mbrl_cem_workspace_bytes(r, rp),
        "mppi": lib.mbrl_mppi_workspace_bytes(r, rm),
        "shard1": lib.mbrl_cem_plan_sharded_workspace_bytes(r, rp, 1),
        "shard8": lib.mbrl_cem_plan_sharded_workspace_bytes(r, rp, 8),
        "batch16": lib.mbrl_cem_plan_batch_workspace_bytes(r, rp, 16),
        "gd1": lib.mbrl_gd_batch_workspace_bytes(r, H, 1),
        "gd16": lib.mbrl_gd_batch_workspace_bytes(r, H, 16),
    }
    with _lib.option("shard_emulate", 1):   # (restored on exit)
        out["shard8_emu"] = lib.mbrl_cem_plan_sharded_workspace_bytes(r, rp, 8)
        # one rank has no peers to emulate: no emulation buffers
        assert lib.mbrl_cem_plan_sharded_workspace_bytes(r, rp, 1) == out["shard1"]
    assert lib.mbrl_get_option(_lib.OPTIONS["shard_emulate"]) == 0
    return out


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_workspace_bytes_are_frozen(name):
    from mbrl_amd import _lib
    lib = _lib.load()
    assert _queries(lib, _lib, name) == EXPECTED[name]


def test_the_table_reaches_every_carver_branch():
    """The cases differ where a carver branches: the pair area (present only for Wpad 512 and at most
    256 pair workgroups), the MPPI plan's second proposal buffer (N * ceil(a / 4) <= 65536), the
    emulation buffers (option set and more than one rank)."""
    from mbrl_amd import _lib
    lib = _lib.load()
    q = {name: _queries(lib, _lib, name) for name in SHAPES}
    a256 = lambda x: (x + 255) // 256 * 256   # noqa: E731
    # cheetah at N = 1024: 64 tiles -> 128 pair workgroups; the area is 129 flag lines, the granules
    # (2 parities x 16 rows x pw = 36 granules of 8 bytes) and the layer columns (2 x 16 x 256 floats)
    pair = 129 * 128 + 128 * 2 * 16 * 36 * 8 + 128 * 2 * 16 * 256 * 4
    s, a, W, L, E = SHAPES["cheetah_n1024"][0]
    N, H, K = SHAPES["cheetah_n1024"][1]
    plain = (a256(E * N * 4) + a256(H * N * a * 4) + 4 * a256(H * a * 4) + a256(H * K * a * 4) + a256(E * H * s * 4) +
             a256(E * 4) + a256(K * 8) + a256(N * 4) + a256(E * 2 * W * 8) + 256 + a256(s * 4))
    assert q["cheetah_n1024"]["cem"] == plain + a256(pair)
    # MPPI: two proposal buffers below the draw threshold, one above it
    assert 4096 * 2 <= 65536 < 32768 * 6
    for name, two in (("cheetah", True), ("humanoid", False)):
        s, a, W, L, E = SHAPES[name][0]
        N, H, K = SHAPES[name][1]
        want = (a256(E * N * 4) + (2 if two else 1) * a256(H * N * a * 4) + 4 * a256(H * a * 4) +
                a256(E * H * s * 4) + a256(E * 2 * W * 8) + 256 + a256(s * 4))
        assert q[name]["mppi"] == want, name
    # emulation: the other ranks' proposals and every iteration's gathered costs
    for name in SHAPES:
        s, a, W, L, E = SHAPES[name][0]
        N, H, K = SHAPES[name][1]
        assert q[name]["shard8_emu"] - q[name]["shard8"] == a256(H * (N // 8) * a * 4) + a256(5 * E * N * 4), name
