"""A CPU restatement of the branch decisions of select_reg_body<KPT> (mujoco-mbrl_amd/csrc/cem.hip), the
register-resident stable top-K behind mbrl_select_elites, cem_update_kernel and cem_select_regen_kernel.

Given the member-mean returns, K, the NaN policy and the member count E, trace() walks the kernel's steps
in vectorised NumPy -- order keys, KPT from N, the key layout, the waves that are full, kmin / kmax, the
wide pass and its bucket, the listed / unlisted decision, the direct rank of a bucket of at most 64 keys,
the 8-bit passes, the final (prefix, kk, eqn, kpad), the compaction -- and returns the elite indices
together with the set of branch labels that input takes. It is a restatement, not instrumentation:
nothing here reads the GPU. Two things pin it to the kernel: tests/test_select_model.py checks that its
constants are the ones in cem.hip and that its elites equal the stable argsort for every row of the
case table (tests/select_cases.py), which a wrong pass arithmetic would break.

Labels:
  kpt{1,2,4,8,16,32}                        the instantiation (smallest power of two with N <= 1024 KPT)
  vec / single                              float4 key layout (KPT >= 4 and N % 4 == 0) or single keys
  load_e1vec / load_general                 the branch-free E == 1 float4 load, or the member-sum load
  load_general_vec / load_general_single      ... and which layout the member-sum load ran in
  waves_all_full / waves_some_partial       N == 1024 KPT, or some wave holds keys past N
  narrow_flat                               all keys equal: no pass
  narrow_wide_only (+ wide_short)           the wide pass resolves every differing bit (fewer than 11)
  narrow_rank64                             wide pass, bucket of at most 64 keys ranked by wave 0
  narrow_list_radix (+ list_two_trips)      wide pass, bucket of 65..SEL_LIST keys listed, 8-bit passes
  narrow_all_radix                          wide pass, bucket above SEL_LIST, 8-bit passes over every key
  radix_short_last_digit                    an 8-bit pass with fewer than 8 bits left
  radix_clustered / radix_mixed             count()'s one-add-per-wave arm / its scattered arm (below)
  compact_bitmap_vec / compact_bitmap_ballot / compact_packed_vec / compact_packed_single
  beany_some / beany_none                   packed float4 compaction: a wave's group with / without a key
                                            equal to the K-th
  ties_all_taken / ties_cut                 two or more keys equal the K-th; all of them elites, or not
  kth_is_pad_key                            the K-th key is NaN under NAN_LAST: the padding key's bits
  nan_first                                 nan_policy == NAN_FIRST

radix_clustered / radix_mixed are claimed only where they are certain. Over every thread's keys the
groups that count() ballots over are known (wave w, key j): a group whose pending keys share one digit
takes the clustered arm, one with several the scattered arm. Over the LDS list the order of the entries
depends on the order of the waves' atomics, so: clustered when every pending key has the same digit,
mixed when the pending keys have more distinct digits than the list has 64-entry chunks (some chunk
then holds two), and neither label otherwise."""
import numpy as np

NAN_LAST, NAN_FIRST = 0, 1            # mbrl.h MBRL_NAN_LAST / MBRL_NAN_FIRST
SEL_WIDE_BITS = 11                    # cem.hip: bits of the wide pass
SEL_LIST = 2048                       # cem.hip: keys of the wide pass's bucket kept in LDS
RANK_MAX = 64                         # cem.hip: `bsz <= 64u`, ranked directly by wave 0
BITMAP_KPT = 8                        # cem.hip: `KPT >= 8 && eqn == kk && prefix != kpad`
KPT_LADDER = (1, 2, 4, 8, 16, 32)     # cem.hip: MBRL_SEL(1) ... MBRL_SEL(32)
ALL_ONES = 0xFFFFFFFF


def order_key(returns, nan_policy=NAN_LAST):
    """uint32 keys whose unsigned order is NumPy's float order: NaN to all ones (NAN_LAST) or 0
    (NAN_FIRST), -0.0 folded onto +0.0, negative values bit-flipped, the others with the sign bit set.
    Subnormals are not zero: they keep their bits."""
    r = np.ascontiguousarray(returns, dtype=np.float32)
    b = r.view(np.uint32).astype(np.int64)
    b[r == 0] = 0
    k = np.where(b >> 31 != 0, ALL_ONES - b, b | 0x80000000)
    k[np.isnan(r)] = ALL_ONES if nan_policy == NAN_LAST else 0
    return k


def kpt_for(N):
    for kpt in KPT_LADDER:
        if N <= 1024 * kpt:
            return kpt
    raise ValueError("N = %d is beyond the register-resident selection" % N)


def layout(N, kpt, vec):
    """(wave, lane, j) of every slot n in [0, 1024 KPT): slots from N on hold the padding key."""
    n = np.arange(1024 * kpt)
    wave, off = n // (64 * kpt), n % (64 * kpt)
    if vec:
        return wave, (off % 256) // 4, 4 * (off // 256) + off % 4
    return wave, off % 64, off // 64


def _kth_bin(hist, kk):
    """First bin whose inclusive count reaches kk; the keys before it."""
    c = np.cumsum(hist)
    b = int(np.searchsorted(c, kk, side="left"))
    return b, int(c[b] - hist[b])


def trace(returns, K, nan_policy=NAN_LAST, E=1):
    """Every decision of select_reg_body for this input, as a dict (labels and elites among them)."""
    returns = np.ascontiguousarray(returns, dtype=np.float32)
    N = returns.shape[0]
    assert returns.ndim == 1 and 1 <= K <= N
    kpt = kpt_for(N)
    vec = kpt >= 4 and N % 4 == 0
    labels = {"kpt%d" % kpt, "vec" if vec else "single"}
    if vec and E == 1:
        labels.add("load_e1vec")
    else:
        labels.update(("load_general", "load_general_vec" if vec else "load_general_single"))
    wfull = 64 * kpt * (np.arange(16) + 1) <= N
    labels.add("waves_all_full" if wfull.all() else "waves_some_partial")
    if nan_policy == NAN_FIRST:
        labels.add("nan_first")

    key = order_key(returns, nan_policy)
    kmin, kmax = int(key.min()), int(key.max())
    key -= kmin
    kpad = ALL_ONES - kmin
    rem = (kmax - kmin).bit_length()                     # 32 - lead
    t = dict(N=N, K=K, E=E, kpt=kpt, vec=vec, wfull=wfull, kmin=kmin, kmax=kmax, lead=32 - rem, rem0=rem,
             kpad=kpad, passes=[])
    mask = (ALL_ONES << rem) & ALL_ONES
    prefix, kk, eqn = 0, K, N
    listed, lst = False, None
    if rem == 0:
        labels.add("narrow_flat")
    else:
        wb = min(SEL_WIDE_BITS, rem)
        wshift = rem - wb
        wmask = (1 << wb) - 1
        if wb < SEL_WIDE_BITS:
            labels.add("wide_short")
        hist = np.bincount((key >> wshift) & wmask, minlength=1 << SEL_WIDE_BITS)
        b, before = _kth_bin(hist, kk)
        prefix |= b << wshift
        mask |= wmask << wshift
        kk -= before
        bsz = eqn = int(hist[b])
        rem = wshift
        t.update(wb=wb, wshift=wshift, bucket=b, bsz=bsz)
        if rem == 0:
            labels.add("narrow_wide_only")
        elif bsz <= SEL_LIST:
            listed, lst = True, key[(key & mask) == prefix]
            assert lst.size == bsz
            if bsz <= RANK_MAX:
                labels.add("narrow_rank64")
                x = int(np.sort(lst)[kk - 1])
                lt, le = int((lst < x).sum()), int((lst <= x).sum())
                prefix, kk, eqn, mask, rem = x, kk - lt, le - lt, ALL_ONES, 0
            else:
                labels.add("narrow_list_radix")
                if bsz > 1024:
                    labels.add("list_two_trips")
        else:
            labels.add("narrow_all_radix")
    if rem > 0:
        wave, _, j = layout(N, kpt, vec)
        gid = (wave * kpt + j)[:N]
    while rem > 0:
        db = min(8, rem)
        shift = rem - db
        dmask = (1 << db) - 1
        if db < 8:
            labels.add("radix_short_last_digit")
        if listed:
            dig = (lst[(lst & mask) == prefix] >> shift) & dmask
            distinct = np.unique(dig).size
            arm = {"radix_clustered"} if distinct == 1 else \
                {"radix_mixed"} if distinct > -(-lst.size // 64) else set()
        else:
            pend = (key & mask) == prefix
            dig = (key[pend] >> shift) & dmask
            lo, hi = np.full(16 * kpt, 256), np.full(16 * kpt, -1)
            np.minimum.at(lo, gid[pend], dig)
            np.maximum.at(hi, gid[pend], dig)
            arm = set()
            if ((hi >= 0) & (lo == hi)).any():
                arm.add("radix_clustered")
            if (lo < hi).any():
                arm.add("radix_mixed")
        labels |= arm
        hist = np.bincount(dig, minlength=256)
        d, before = _kth_bin(hist, kk)
        prefix |= d << shift
        mask |= dmask << shift
        kk -= before
        eqn = int(hist[d])
        rem = shift
        t["passes"].append(dict(db=db, shift=shift, pending=int(dig.size), digits=int(np.unique(dig).size),
                                arm=sorted(arm)))

    kth_pad = prefix == kpad
    if kth_pad:
        labels.add("kth_is_pad_key")
    if eqn >= 2:
        labels.add("ties_all_taken" if eqn == kk else "ties_cut")
    if kpt >= BITMAP_KPT and eqn == kk and not kth_pad:
        labels.add("compact_bitmap_vec" if vec else "compact_bitmap_ballot")
    elif vec:
        labels.add("compact_packed_vec")
        slots = np.full(1024 * kpt, kpad)
        slots[:N] = key
        wave, _, j = layout(N, kpt, vec)
        beany = np.zeros(16 * kpt // 4, dtype=bool)
        np.logical_or.at(beany, wave * (kpt // 4) + j // 4, slots == prefix)
        if beany.any():
            labels.add("beany_some")
        if not beany.all():
            labels.add("beany_none")
    else:
        labels.add("compact_packed_single")
    eq = key == prefix
    take = (key < prefix) | (eq & (np.cumsum(eq) <= kk))
    elites = np.nonzero(take)[0].astype(np.int64)
    assert elites.size == K and int(eq.sum()) == eqn and 1 <= kk <= eqn
    t.update(prefix=prefix, kk=kk, eqn=eqn, listed=listed, labels=labels, elites=elites)
    return t


def select_model(returns, K, nan_policy=NAN_LAST, E=1):
    """(elite indices in ascending order, the branch labels select_reg_body takes for this input)."""
    t = trace(returns, K, nan_policy, E)
    return t["elites"], frozenset(t["labels"])


def update_fits(N, K, a):
    """cem.hip update_kpt() != 0: the selection fits registers and select / refit fit 160 KiB of LDS."""
    if a > 64 or K < 1 or K > N or N > 1024 * KPT_LADDER[-1]:
        return False
    a4 = (a + 3) & ~3
    sel = 2 * 16 * 257 + (1 << SEL_WIDE_BITS) + SEL_LIST + 4                  # sel_words()
    nch = (K + 31) // 32                                                      # ELITE_CHUNK = 32
    ref = ((nch * 33 * a + 3) & ~3) + ((nch * a + 3) & ~3) + 3 * a4           # refit_rows_floats()
    return (((K + 3) & ~3) + 2 * a4 + max(sel, ref)) * 4 + 1024 <= 160 * 1024
