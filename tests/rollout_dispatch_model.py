"""A CPU restatement of which fp32 rollout kernel a model shape runs, and whether it runs at all.

Four pieces of the HIP extension's host code, in plain Python:
  geometry()          make_geometry (mujoco-mbrl_amd/csrc/mbrl_internal.h): T, Wpad, K0C, NOT, lda, pw and the
                      packed member stride with every optional stream (split, m8, m4)
  lds_floats/_bytes   lds_map / rollout_lds_bytes (same header): the dynamic LDS of a workgroup of M rows
  dispatch()          the fp32 part of rollout_impl (csrc/plan.hip) and launch_rollout (csrc/rollout.hip):
                      R, NW, part_alias, ring or generic, the half-group seam, the R = 2 -> 1 fallbacks, the
                      refusals, and the 8-candidate branch as a function of an explicit CU count
  trajectory_instance() traj_impl (csrc/plan.hip) and the launchers of csrc/traj.hip: traj_reg_supported,
                      launch_reg_w / launch_reg_k0, coop_k0r, the static half of traj_coop_supported,
                      launch_coop_width and launch_coop_variant's grid choice -> the kernel with its template
                      arguments (pinned by tests/test_traj_cases_host.py and, through the hand-off block each
                      kernel leaves in the workspace, tests/test_gpu_traj_envelope.py)
  trajectory_kernel() the kernel family alone: 'reg', 'coop' or 'plain'

dispatch() returns an Instance (hashable: the template arguments of the kernel that runs, plus the labels a
coverage test wants) or a Refusal (the MBRL_* code and a fragment of the message). It is a restatement, not
instrumentation: nothing here reads the GPU. What pins it: tests/test_rollout_dispatch_model.py compares
the member stride with mbrl_mlp_packed_bytes over the case table and random shapes (host-only, the geometry
half) and checks the constants against the sources; tests/test_gpu_envelope.py runs the table on the GPU,
where a shape the model calls refused must be refused with that message and one it calls accepted must run
and match the oracle (the LDS half).

  split_kernel()      the F16X3 / F16X6 block of rollout_impl (the `g.precision` branch), make_geometry's K0S /
                      NOS / CS with the parity bump, rollout_split_supported, split_lds / rollout_split_lds_bytes
                      and split_ts (csrc/rollout_f16x3.hip), and the redo pass's rollout_lds_bytes(X, 32) check

Not modelled: the column-split pairs (a plan's workspace offers them only at Wpad = 512 with at most 256
workgroups; a lone mbrl_rollout_cost never) and the opt-in 4-candidate tile.
"""
from collections import namedtuple

MAX_LAYERS = 4                 # mbrl_internal.h
MAX_T = 16                     # make_geometry: `if (T > 16) return false;`
LDS_LIMIT = 160 * 1024         # plan.hip: `> 160 * 1024`
LDS_FLOOR = 82 * 1024          # rollout_lds_bytes: one workgroup per CU
ACTION_SLOTS = 768             # plan.hip: `16 * g.a > 768`, `16 * R * g.a > 768`
R2_MIN_N = 2 * 16 * 256        # plan.hip: 32-candidate tiles from N = 8192
RING_SHAPES = ((2, 2), (6, 6), (2, 6), (6, 2))   # rollout.hip launch_rollout_tn
CASES = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (1, 2), (2, 2), (4, 2), (8, 2))   # rollout.hip MBRL_CASE
MI355X_CUS = 256

MBRL_EUNSUPPORTED = -2

Instance = namedtuple("Instance", "kernel T R NW K0C_T NOT_T GS part_alias reward fallback lds_bytes")
Refusal = namedtuple("Refusal", "code fragment lds_bytes")


def _even(x):
    return (x + 1) & ~1


def _r4(x):
    return (x + 3) & ~3


def _r64(x):
    return (x + 63) // 64 * 64


def geometry(s, a, W, L, E=1, reward=0):
    """make_geometry: a dict, or None where it returns false."""
    reward = int(bool(reward))
    if s < 1 or a < 1 or W < 1 or L < 1 or L > MAX_LAYERS or E < 1:
        return None
    T = 1
    while 64 * T < W:
        T *= 2
    if T > MAX_T:
        return None
    g = dict(s=s, a=a, W=W, L=L, E=E, reward=reward, so=s + reward, T=T, Wpad=64 * T)
    g["K0C"] = _even((s + a + 15) // 16)
    g["NOT"] = _even((g["so"] + 15) // 16)
    if g["NOT"] > 2 * 4 * T * 4:
        return None
    g["C"] = g["K0C"] + (L - 1) * 4 * T + g["NOT"]
    k0 = 16 * g["K0C"]
    g["lda"] = max(g["Wpad"], k0) + 4
    g["pw"] = 16 * g["NOT"] + 4
    stream = g["C"] * 1024 * T
    bias = L * g["Wpad"] + 16 * g["NOT"]
    tw = (s + a) * g["Wpad"] + (L - 1) * W * g["Wpad"] + g["so"] * W
    end = stream + bias + tw
    split_ok = T in (4, 8)
    K0S, NOS = (s + a + 31) // 32, g["NOT"] // 2
    if (K0S + NOS) & 1:
        K0S += 1
    CS = K0S + (L - 1) * 2 * T + NOS
    if split_ok:
        end = _r64(end) + (CS * 2048 * T + 64) + (CS * 3072 * T + 64)
    g["m8_ok"] = split_ok and not reward and g["K0C"] in (2, 6) and g["NOT"] in (2, 6)
    NOP8 = (g["NOT"] // 2 + 1) // 2
    NOC8 = 2 if g["NOT"] == 2 else 4 * NOP8
    if g["m8_ok"]:
        end = _r64(end) + (g["K0C"] + (L - 1) * 4 * T + NOC8) * 1024 * T
    g["m4_ok"] = g["m8_ok"] and (g["so"] + 15) // 16 <= 4
    if g["m4_ok"]:
        end = _r64(end) + (g["K0C"] + (L - 1) * 4 * T + 4) * 1024 * T
    g["member_stride"] = _r64(end)     # floats per ensemble member
    return g


def lds_floats(g, M, nw, part_alias):
    """lds_map(...).total_floats for a workgroup of M candidate rows."""
    s, a = g["s"], g["a"]
    o = 2 * _r4(M * g["lda"])                                  # act, act2
    if not part_alias:
        o += _r4(max(nw, 4) * M * g["pw"])                     # part
    o += _r4(M * s) + _r4(2 * M * a)                           # sterm, aterm
    o += 4 * _r4(s) + 2 * _r4(a)                               # obs_mean, obs_std, goal, cw; act_mean, act_std
    o += _r4(g["L"] * g["Wpad"] + 16 * g["NOT"]) + _r4(16)     # hbias, lflag
    return o


def lds_need_bytes(g, M, nw, part_alias):
    """What rollout_impl compares with 160 KiB (the 82 KiB floor of rollout_lds_bytes never decides it)."""
    return 4 * lds_floats(g, M, nw, part_alias)


def lds_launch_bytes(g, M, nw, part_alias):
    return max(lds_need_bytes(g, M, nw, part_alias), LDS_FLOOR)


def _alias_ok(g, nw):
    return not g["reward"] and g["L"] >= 3 and g["L"] % 2 == 1 and max(nw, 4) * g["pw"] <= g["lda"]


def dispatch(s, a, W, L, E=1, reward=0, *, N, cus=MI355X_CUS, rollout_tile=0, group_seam=0):
    """The fp32 kernel instance mbrl_rollout_cost launches for N candidates on a device of `cus` compute
    units, or the refusal. rollout_tile / group_seam: the MBRL_OPT_* switches of those names (0 = auto)."""
    g = geometry(s, a, W, L, E, reward)
    if g is None:
        return Refusal(MBRL_EUNSUPPORTED, "unsupported MLP shape", None)
    if 16 * a > ACTION_SLOTS:
        return Refusal(MBRL_EUNSUPPORTED, "action_dim %d too large (max 48)" % a, None)
    T = g["T"]
    if lds_need_bytes(g, 16, 8 if T >= 2 else 4, _alias_ok(g, 8 if T >= 2 else 4)) > LDS_LIMIT:
        need = lds_need_bytes(g, 16, 8 if T >= 2 else 4, _alias_ok(g, 8 if T >= 2 else 4))
        return Refusal(MBRL_EUNSUPPORTED, "LDS footprint %d B exceeds 160 KiB" % need, need)
    gs_auto = T == 8 and g["K0C"] == 2 and g["NOT"] == 2
    seam = group_seam == 1 or (group_seam == 0 and gs_auto)
    R = 2 if (N >= R2_MIN_N and T <= 8) else 1
    fallback = None
    if 16 * R * a > ACTION_SLOTS:
        R, fallback = 1, "actions"
    nw = 8 if (R == 1 and T >= 2) else 4
    if g["m8_ok"]:
        use8 = ((N + 15) // 16) * E * 2 <= cus
        if rollout_tile:
            use8 = rollout_tile in (8, 4)
        if use8 and lds_need_bytes(g, 8, nw, False) <= LDS_LIMIT:
            return Instance("m8", T, 0, 8, g["K0C"], g["NOT"], False, False, 0, None,
                            lds_launch_bytes(g, 8, 8, False))
    if R == 2 and T >= 2 and not g["reward"] and L >= 3 and L % 2 == 1 and 8 * g["pw"] <= g["lda"]:
        nw = 8
    alias = _alias_ok(g, nw)
    if lds_need_bytes(g, 16 * R, nw, alias) > LDS_LIMIT:
        R, fallback = 1, "lds"
        nw = 8 if T >= 2 else 4
        alias = _alias_ok(g, nw)
        assert lds_need_bytes(g, 16, nw, alias) <= LDS_LIMIT     # the refusal above
    assert (T, R) in CASES
    # launch_rollout_t / _tn / _tr
    NW = 8 if (R == 2 and T >= 2 and nw == 8) else (8 if (T >= 2 and R == 1) else 4)
    ring = 4 * T // NW <= 8 and (g["K0C"], g["NOT"]) in RING_SHAPES
    k0c_t, not_t = (g["K0C"], g["NOT"]) if ring else (0, 0)
    GS = bool(ring and NW == 8 and T <= 8 and seam)
    return Instance("m16", T, R, NW, k0c_t, not_t, GS, bool(alias), g["reward"], fallback,
                    lds_launch_bytes(g, 16 * R, NW, alias))


# ---- the split-operand kernels (rollout_f16x3.hip): precision F16X3 (P = 2) / F16X6 (P = 3)
SPLIT_SHAPES = ((1, 1), (2, 2), (3, 1), (1, 3), (3, 3))   # MBRL_SPLIT_SHAPES: (K0S, NOS)
SPLIT_T = (4, 8)               # make_geometry split_ok, rollout_split_supported
SPLIT_MAX_A = 48               # 16 * SMAXA
SPLIT_R2_MIN_N = 256 * 32      # plan.hip: `int RS = N >= 256 * 32 ? 2 : 1;`
SPLIT_WAVES = 8                # SW

Split = namedtuple("Split", "kind T R P K0S NOS TS lds_bytes")
F32 = namedtuple("F32", "kind reason")


def split_geometry(g):
    """make_geometry's split fields: (K0S, NOS, CS); K0S + NOS is made even by a zero-padded layer-0 chunk."""
    K0S, NOS = (g["s"] + g["a"] + 31) // 32, g["NOT"] // 2
    if (K0S + NOS) & 1:
        K0S += 1
    return K0S, NOS, K0S + (g["L"] - 1) * 2 * g["T"] + NOS


def split_ts(R, P, K0S, NOS):
    """split_ts: tiles per weight ring slot."""
    return 2 if (P == 2 or (R == 1 and K0S <= 2 and NOS <= 2)) else 1


def split_lds_need_bytes(g, R, P):
    """split_lds(...).bytes: every block rounded up to 16 bytes."""
    r16 = lambda b: (b + 15) & ~15  # noqa: E731
    K0S = split_geometry(g)[0]
    M, sr = 16 * R, P * max(g["Wpad"], 32 * K0S) + 8
    o = r16(M * sr * 2) * (2 if R == 1 else 1)                # x, y (R = 2: one buffer)
    o += r16(SPLIT_WAVES * M * g["pw"] * 4) + r16(2 * M * 4)  # part, acs
    o += 4 * r16(g["s"] * 4) + 2 * r16(g["a"] * 4)            # obs_mean, obs_std, goal, cw; act_mean, act_std
    o += r16((g["L"] * g["Wpad"] + 16 * g["NOT"]) * 4) + r16(16)   # hbias, flag
    return o


def _split_refusal(g, R, P):
    """rollout_split_supported, as the reason it returns false for (None: supported)."""
    K0S, NOS, CS = split_geometry(g)
    if R != 1 and not (R == 2 and g["NOT"] == 2):
        return "R = 2 needs one output chunk"
    if g["reward"] or g["T"] not in SPLIT_T or g["a"] > SPLIT_MAX_A:
        return "reward, T or a"
    assert g["s"] <= 16 * g["NOT"] and g["NOT"] == 2 * (CS - K0S - (g["L"] - 1) * 2 * g["T"])
    if max(split_lds_need_bytes(g, R, P), LDS_FLOOR) > LDS_LIMIT:
        return "split LDS"
    if (K0S, NOS) not in SPLIT_SHAPES:
        return "shape class (%d, %d)" % (K0S, NOS)
    return None


def split_kernel(s, a, W, L, E=1, reward=0, *, N, P, split_tile=0):
    """What mbrl_rollout_cost launches for a problem of precision F16X3 (P = 2) or F16X6 (P = 3):
    Split("split", T, R, P, K0S, NOS, TS, lds_bytes) -- the template arguments of rollout_split_kernel and
    its dynamic LDS -- or F32("f32", reason): the fp32 path alone (dispatch() says which kernel, or that
    the call is refused). split_tile: MBRL_OPT_SPLIT_TILE (0 auto, 16, 32)."""
    assert P in (2, 3)
    g = geometry(s, a, W, L, E, reward)
    nw16 = 8 if g is not None and g["T"] >= 2 else 4
    if g is None or 16 * a > ACTION_SLOTS or lds_need_bytes(g, 16, nw16, _alias_ok(g, nw16)) > LDS_LIMIT:
        return F32("f32", "refused")        # dispatch()'s three refusals: rollout_validate comes first
    if g["T"] not in SPLIT_T:
        return F32("f32", "T = %d" % g["T"])
    if g["reward"]:
        return F32("f32", "reward head")
    R = 2 if N >= SPLIT_R2_MIN_N else 1
    if split_tile:
        R = 2 if split_tile == 32 else 1
    # the redo pass at 32 rows: 4 waves, partials not aliased (part_alias is set after this block)
    if R == 2 and (_split_refusal(g, 2, P) or lds_launch_bytes(g, 32, 4, False) > LDS_LIMIT):
        R = 1
    why = _split_refusal(g, R, P)
    if why:
        return F32("f32", why)
    K0S, NOS, _ = split_geometry(g)
    return Split("split", g["T"], R, P, K0S, NOS, split_ts(R, P, K0S, NOS),
                 max(split_lds_need_bytes(g, R, P), LDS_FLOOR))


# ---- the single-trajectory kernels (traj.hip, dispatched by traj_impl in plan.hip)
COOP_ROWS, COOP_MAX_W, COOP_LDS_LIMIT = 16, 512, 150 * 1024
COOP_MAX_GRID = 1024           # traj_coop_supported: `P * E > 1024`
COOP_BUDGETS = ((32, 32, 2), (96, 80, 5))    # coop_k0r / launch_traj_coop: (K0R, largest s, SM); 16 SM >= s
XCD_MAX_E = 8                  # launch_coop_variant: the per-XCD grid needs `E <= 8`
REG_MAX_W = 256                # traj_reg_supported: `A.Wpad > 256`
REG_K0_SPLIT = 8               # launch_reg_k0: `K0 <= 8` runs the K0R = 8 instance, else K0R = 32
REG_LDS_LIMIT = 64 * 1024      # traj_reg_supported
REG_FIXED_FLOATS = 32 + 32 + 128     # traj_reg_kernel's x0, out and prm blocks (beside 2 Wpad and H a)
TRAJ_HOP_DEFAULT = 2           # mbrl_host.h kTrajHopDefault: TrajArgs.hop_mode under MBRL_OPT_TRAJ_HOP = 0

Reg = namedtuple("Reg", "kernel WP NHL K0R")
Coop = namedtuple("Coop", "kernel K0R SM WI grid hop")     # grid "xcd" / "pe"; hop: TrajArgs.hop_mode as launched
Plain = namedtuple("Plain", "kernel gated")

# every instance launch_traj_reg / launch_traj_coop list
REG_INSTANCES = frozenset((wp, nhl, k0r) for wp in (64, 128, 256) for nhl in range(4) for k0r in (8, 32)
                          if wp <= 128 or nhl <= 1)
COOP_INSTANCES = frozenset((k0r, sm, wi) for k0r, _, sm in COOP_BUDGETS for wi in (2, 4, 8, 16))


def _reg_max_hidden(Wp):
    return 3 if Wp <= 128 else (1 if Wp <= 256 else 0)


def _coop_k0r(s, a):
    for k0r, max_s, _ in COOP_BUDGETS:
        if s + a <= k0r and s <= max_s:
            return k0r
    return 0


def _coop_lds_bytes(s, a, W, Wp, L, H, k0r):
    o = (L - 1) * COOP_ROWS * (W + 32) + _r4(max(k0r, s + a)) + 2 * Wp + _r4(s) + _r4(H * a)
    o += _r4((L - 1) * COOP_ROWS) + 3 * _r4(s) + 4
    return 4 * o


def reg_max_steps(a, Wp):
    """The longest H traj_reg_supported admits: H a <= 16384 - 192 - 2 Wpad floats of normalised actions."""
    return (REG_LDS_LIMIT // 4 - REG_FIXED_FLOATS - 2 * Wp) // a


def _reg_supported(s, a, Wp, L, H):
    return Wp <= REG_MAX_W and L - 1 <= _reg_max_hidden(Wp) and s + a <= 32 and s <= 32 and \
        4 * (REG_FIXED_FLOATS + 2 * Wp + H * a) <= REG_LDS_LIMIT


def _coop_supported(s, a, W, Wp, L, E, H):
    """The static half of traj_coop_supported (grid_fits, the device's occupancy, is left out)."""
    k0r = _coop_k0r(s, a)
    return bool(k0r) and L >= 2 and W == Wp and Wp <= COOP_MAX_W and (Wp // COOP_ROWS) * E <= COOP_MAX_GRID and \
        _coop_lds_bytes(s, a, W, Wp, L, H, k0r) <= COOP_LDS_LIMIT


def trajectory_instance(s, a, W, L, E=1, *, H, traj_hop=0, debug_abort=0):
    """The kernel mbrl_trajectory / final_trajectory launches for one action sequence, with its template
    arguments: Reg("reg", WP, NHL, K0R), Coop("coop", K0R, SM, WI, grid, hop) or Plain("plain", gated), None
    where make_geometry refuses the shape. traj_hop / debug_abort: MBRL_OPT_TRAJ_HOP / MBRL_OPT_DEBUG_TRAJ_ABORT.

    traj_reg_supported, launch_reg_w / launch_reg_k0, coop_k0r, traj_coop_supported, launch_coop_width and the
    grid choice of launch_coop_variant, without their occupancy half (grid_fits: only the device knows; on a
    device whose occupancy refuses the grid, Coop becomes Plain ungated, and "xcd" becomes "pe"). With
    debug_abort the register kernel is skipped; a cooperative launch then sets the status word and returns,
    and the answer is the gated plain kernel behind it, which computes the states."""
    g = geometry(s, a, W, L, E)
    if g is None:
        return None
    Wp = g["Wpad"]
    if _reg_supported(s, a, Wp, L, H) and not debug_abort:
        return Reg("reg", Wp, L - 1, 8 if s + a <= REG_K0_SPLIT else 32)
    if _coop_supported(s, a, W, Wp, L, E, H):
        if debug_abort:
            return Plain("plain", True)
        k0r = _coop_k0r(s, a)
        sm = dict((k, m) for k, _, m in COOP_BUDGETS)[k0r]
        hop = TRAJ_HOP_DEFAULT if traj_hop == 0 else traj_hop - 1
        if hop >= 1 and E <= XCD_MAX_E:
            return Coop("coop", k0r, sm, Wp // 32, "xcd", hop)
        return Coop("coop", k0r, sm, Wp // 32, "pe", 0)
    return Plain("plain", False)


def trajectory_kernel(s, a, W, L, E=1, reward=0, *, H):
    """'reg', 'coop' (where the workspace and the device's occupancy also allow it) or 'plain'."""
    if geometry(s, a, W, L, E, reward) is None:
        return None
    return trajectory_instance(s, a, W, L, E, H=H).kernel
