"""CPU: the inputs of tests/test_gpu_spec_edges.py and a guard that they contain what they claim to cover.

spec_gemm_kernel (csrc/spec.hip) lays the 64-frame tiles of all clips of a call out in one flat list and gives block g
of G the tiles [g q, (g + 1) q), q = ceil(tiles / G).  Everything subtle in it -- the (count, mean, M2) carried from
tile to tile, the flush to partial slot clip + block when the clip changes under a block, the skip over clips that own
no tile, the frame count spec_finish_kernel re-derives per slot -- only runs for q >= 2, and G follows the device
(2 x CUs = 512 on an MI355X), so the GPU tests force G through xm_debug_set("spec_blocks", v).  `plan` below restates
the launch geometry in numpy; the tests here run it over the tables and the G values of the GPU tests and assert that
a block spans several clips, a clip several blocks, a block starts behind zero-frame clips, ... -- on a machine without
a GPU, so that an edit of a table cannot quietly turn the GPU cases back into one tile per block."""
import numpy as np

from oracle import oracle as O
from test_gpu_spec_bucket import NS, NW, TOL, _bank, _len

FT = 64                      # kSpecFT: frames per tile
G_MI355X = 512               # the default grid on 256 CUs (kSpecOcc = 2)
EPS = 2.0 ** -24             # half an fp32 ulp of 1


# ---- the launch geometry, restated --------------------------------------------------------------------------------
def frames_of(lengths, nw=NW, ns=NS):
    """spec_frames: T = floor((len - Nw) / Ns) + 1, 0 for a clip shorter than one frame"""
    ln = np.asarray(lengths, np.int64)
    return np.where(ln >= nw, (ln - nw) // ns + 1, 0)


def plan(T, G):
    """(tile_start, q, blocks): blocks[g] = [(clip, first tile, end tile)] in the order block g meets them, tiles
    counted inside the clip; an idle block has an empty list"""
    T = np.asarray(T, np.int64)
    tiles = (T + FT - 1) // FT
    start = np.concatenate([[0], np.cumsum(tiles)])
    total = int(start[-1])
    q = -(-total // G)
    blocks = []
    for g in range(G):
        w0, w1 = g * q, min((g + 1) * q, total)
        runs = []
        for w in range(w0, w1):
            n = int(np.searchsorted(start, w, side="right")) - 1
            if runs and runs[-1][0] == n:
                runs[-1][2] += 1
            else:
                runs.append([n, w - int(start[n]), w - int(start[n]) + 1])
        blocks.append([tuple(r) for r in runs])
    return start, q, blocks


def last_tile_frames(T):
    """valid frames in the last tile of every clip that owns one"""
    return sorted({int(t - (t - 1) // FT * FT) for t in np.asarray(T) if t > 0})


def check_slots(T, G):
    """partial slot clip + block: distinct over all (block, clip) pairs, below N + G, and the frames the finish kernel
    derives for them from (lo, hi, T) add up to T"""
    start, q, blocks = plan(T, G)
    slots = [n + g for g, runs in enumerate(blocks) for n, _, _ in runs]
    assert len(slots) == len(set(slots)) and (not slots or max(slots) < len(T) + G), (G, slots)
    seen = np.zeros(len(T), np.int64)
    for runs in blocks:
        for n, a, b in runs:
            seen[n] += min(b * FT, int(T[n])) - a * FT
    assert seen.tolist() == [int(t) for t in T], G


def block_after_empty(T, G):
    """blocks whose first tile is the first tile of a clip that follows one or more zero-frame clips"""
    _, _, blocks = plan(T, G)
    return [g for g, runs in enumerate(blocks) if runs and runs[0][1] == 0 and runs[0][0] > 0 and T[runs[0][0] - 1] == 0]


# ---- (a) / (d): many tiles per block, blocks across clips ----------------------------------------------------------
# one-tile, two-tile and multi-tile clips; residual samples 0, 1, 159 as in test_gpu_spec_bucket.py
TABLE_A = [(64, 159), (65, 0), (100, 159), (129, 1), (157, 0), (199, 0), (257, 1), (31, 159), (128, 0), (70, 0), (321, 1),
           (33, 159), (160, 0)]
RSIZE_A = 31
TILES_A = 35
FORCED_A = [1, 2, 3, 5, 7, TILES_A - 1, TILES_A, TILES_A + 3]        # and 0, the default


def table_a():
    """(bank, desc N x 3 int64 host) with the window at the start, the centre and the end of the clip in turn"""
    bank, offs = _bank(TABLE_A, 31)
    T = np.array([t for t, _ in TABLE_A])
    f0 = np.where(np.arange(len(T)) % 3 == 0, 0, np.where(np.arange(len(T)) % 3 == 1, (T - RSIZE_A) // 2, T - RSIZE_A))
    return bank, np.stack([offs[:-1], np.diff(offs), f0], 1).astype(np.int64)


D_CLIP, D_AT = 4, (0, 6, 15)   # (d): clip 4 of (a) (T = 157, three tiles) first, in the middle and last
FORCED_D = [1, 3]


def table_d():
    bank, desc = table_a()
    rows = [desc[D_CLIP]] + list(desc[:5]) + [desc[D_CLIP]] + list(desc[5:]) + [desc[D_CLIP]]
    return bank, np.stack(rows).astype(np.int64)


# ---- (b): short, empty and overhanging clips ----------------------------------------------------------------------
RSIZE_B = 8
SEED_B = 5
# (len, which f0 of (-2, 0, T - 3)); zero-frame clips first, last, twice in a row in the middle, and in front of the
# clip whose first tile is the first tile of block 1 for G = 2 (tile 8) and of blocks 1 and 2 for G = 3 (tiles 6, 12)
TABLE_B = [(0, 1), (_len(2), 0), (_len(3, 1), 1), (_len(5), 2), (NW, 1), (_len(31, 159), 0), (_len(32), 2), (NW - 1, 2),
           (_len(63, 1), 0), (NW - 1, 0), (_len(33), 1), (0, 2), (NW - 1, 1), (_len(64, 159), 2), (_len(2, 159), 2),
           (_len(65), 0), (0, 0), (_len(3), 0), (_len(5, 1), 1), (_len(65, 1), 2), (NW - 1, 0)]
FORCED_B = [1, 2, 3]
KAPPA_CAP = {2: 4000.0, 3: 200.0, 5: 40.0}
TABLE_B0 = [0, NW - 1, 100, 0, NW - 1]                               # the call in which no clip has a frame


def bank_of(lengths, seed):
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return (rng.standard_normal(int(offs[-1])) * 0.1).astype(np.float32), offs


def table_b():
    lengths = [ln for ln, _ in TABLE_B]
    bank, offs = bank_of(lengths, SEED_B)
    T = frames_of(lengths)
    f0 = np.array([(-2, 0, int(t) - 3)[w] for t, (_, w) in zip(T, TABLE_B)])
    return bank, np.stack([offs[:-1], lengths, f0], 1).astype(np.int64)


# ---- (e): more clips than spec_plan_kernel has threads --------------------------------------------------------------
N_E, RSIZE_E = 1030, 4


def table_e():
    rng = np.random.default_rng(77)
    T = rng.choice([5, 31, 33, 64, 65, 65], N_E)
    T[rng.choice(N_E, 20, replace=False)] = 0
    T[[0, 1023, 1024, 1025, N_E - 1]] = [65, 33, 0, 65, 5]           # the seam between threads 511 and 512 of the plan
    lengths = np.where(T > 0, NW + NS * (T - 1) + rng.integers(0, NS, N_E), rng.integers(0, NW, N_E))
    bank, offs = bank_of(lengths, 78)
    f0 = np.array([(-2, 0, int(t) - 3)[i % 3] for i, t in enumerate(T)])
    return bank, np.stack([offs[:-1], lengths, f0], 1).astype(np.int64)


# ---- the float64 reference with the header's fill ------------------------------------------------------------------
def reference(bank, desc, rsize, **audio):
    """per clip (ref 512 x rsize float64 or None for T < 2, kappa): O.spec_rownorm(O.run_spec(clip)) cropped at f0;
    frames of the crop outside [0, T) count as magnitude 0, i.e. (0 - mu) / sd.  kappa = max over the bins of mu / sd,
    by which the fp32 rounding of a magnitude is amplified"""
    a = dict(fs=16000, Tw=25, Ts=10)
    a.update(audio)
    nw, ns = int(round(1e-3 * a["Tw"] * a["fs"])), int(round(1e-3 * a["Ts"] * a["fs"]))
    out = []
    for src, ln, f0 in np.asarray(desc).tolist():
        T = int(frames_of([ln], nw, ns)[0])
        if T < 2:
            out.append((None, 0.0))
            continue
        mag = O.run_spec(bank[src:src + ln], a["fs"], a["Tw"], a["Ts"])
        norm = O.spec_rownorm(mag)[:, :, 0, 0].astype(np.float64)
        m = mag[:, :, 0, 0].astype(np.float64)
        mu, sd = m.mean(1), m.std(1, ddof=1)
        ref = np.repeat(((0.0 - mu) / sd)[:, None], rsize, 1)
        i = np.arange(rsize)
        ok = (f0 + i >= 0) & (f0 + i < T)
        ref[:, ok] = norm[:, f0 + i[ok]]
        out.append((ref, float((mu / sd).max())))
    return out


def allowance(T, kappa):
    """TOL, the allowance of this path; for T < 31 a row can have sd << mu, and the fp32 rounding of mu and of each
    magnitude (about four ulps of a magnitude -- the kernel's own comment measures two -- plus the rounding of mu,
    doubled) is amplified by kappa"""
    return max(TOL, 8 * EPS * kappa) if T < 31 else TOL


def regroup_bound(ref, kappa):
    """two groupings of a clip's partial statistics differ in the order of fp64 merges only, so mu and 1 / sd each move
    by at most one fp32 ulp: out = (mag - mu) inv moves by at most 2^-22 (kappa + max |out|)"""
    return 2.0 ** -22 * (kappa + float(np.abs(ref).max()))


# ---- the guard ---------------------------------------------------------------------------------------------------------
def test_plan_restatement():
    start, q, blocks = plan([64, 0, 65, 130, 0, 0, 1], 3)
    assert start.tolist() == [0, 1, 1, 3, 6, 6, 6, 7] and q == 3
    assert blocks == [[(0, 0, 1), (2, 0, 2)], [(3, 0, 3)], [(6, 0, 1)]]
    assert plan([0, 0], 4)[1] == 0 and plan([0, 0], 4)[2] == [[], [], [], []]
    assert last_tile_frames([64, 0, 65, 130, 1, 97]) == [1, 2, 33, 64]
    assert block_after_empty([64, 0, 65, 130, 0, 0, 1], 3) == [2]


def test_table_a_covers_what_it_claims():
    bank, desc = table_a()
    T = frames_of(desc[:, 1])
    assert T.tolist() == [t for t, _ in TABLE_A] and (desc[:, 2] >= 0).all() and (desc[:, 2] + RSIZE_A <= T).all()
    assert sorted({int(r) for r in desc[:, 1] - NW - NS * (T - 1)}) == [0, 1, 159]
    assert {0, int(T[1] - RSIZE_A) // 2, int(T[2] - RSIZE_A)} <= set(desc[:3, 2].tolist())
    start, _, _ = plan(T, 1)
    assert int(start[-1]) == TILES_A and desc[-1, 0] + desc[-1, 1] == bank.size
    tiles = np.diff(start)
    assert {1, 2} <= set(tiles.tolist()) and tiles.max() >= 5
    assert {1, 31, 32, 33} <= set(last_tile_frames(T))
    spans3, clip3, on_boundary, idle = set(), set(), set(), set()
    for G in FORCED_A + [G_MI355X]:
        _, q, blocks = plan(T, G)
        check_slots(T, G)
        per_clip = np.zeros(len(T), int)
        for g, runs in enumerate(blocks):
            if not runs:
                idle.add(G)
            if len(runs) >= 3:
                spans3.add(G)
            if q >= 2 and runs and runs[-1][2] == tiles[runs[-1][0]] and g * q + q < TILES_A:
                on_boundary.add(G)
            for n, _, _ in runs:
                per_clip[n] += 1
        if per_clip.max() >= 3 and q >= 2:
            clip3.add(G)
    print("spans >= 3 clips:", sorted(spans3), "clip over >= 3 blocks:", sorted(clip3), "ends on a boundary:",
          sorted(on_boundary), "idle:", sorted(idle))
    assert {1, 2, 3, 5, 7} <= spans3 and clip3 and on_boundary
    assert {TILES_A - 1, TILES_A + 3, G_MI355X} <= idle and TILES_A not in idle
    assert all(plan(T, G)[1] >= 2 for G in (1, 2, 3, 5, 7, TILES_A - 1))


def test_table_d_moves_the_copies():
    _, desc = table_d()
    assert all((desc[i] == desc[D_AT[0]]).all() for i in D_AT) and D_AT[-1] == len(desc) - 1
    T = frames_of(desc[:, 1])
    _, q, blocks = plan(T, 3)
    cuts = [tuple((g, a, b) for g, runs in enumerate(blocks) for n, a, b in runs if n == i) for i in D_AT]
    print("the copies under G = 3:", cuts)
    assert q >= 2 and len({tuple((a, b) for _, a, b in c) for c in cuts}) >= 2       # not cut at the same tiles
    for G in FORCED_D + [G_MI355X]:
        check_slots(T, G)


def test_table_b_covers_what_it_claims():
    bank, desc = table_b()
    ln, T = desc[:, 1], frames_of(desc[:, 1])
    assert {0, NW - 1} <= set(ln[T == 0].tolist()) and NW in ln.tolist()
    assert {1, 2, 3, 5, 31, 32, 33, 63, 64, 65} <= set(T.tolist())
    assert T[0] == 0 and T[-1] == 0 and any(T[i] == 0 and T[i + 1] == 0 for i in range(1, len(T) - 2))
    assert {1, 31, 32, 33} <= set(last_tile_frames(T))
    for t in (2, 3, 5, 65):                                  # crops that overhang in front, behind, and not at all
        assert {-2, 0, t - 3} & set(desc[T == t, 2].tolist()) and (desc[T == t, 2] + RSIZE_B > t).any()
    assert (desc[:, 2] == -2).any() and (desc[:, 2] == 0).any()
    for G in FORCED_B + [G_MI355X]:
        check_slots(T, G)
    assert plan(T, 2)[1] >= 2 and plan(T, 3)[1] >= 2
    assert block_after_empty(T, 2) == [0, 1] and block_after_empty(T, 3) == [0, 1, 2]
    assert any(len(runs) >= 3 for runs in plan(T, 3)[2])
    assert (frames_of(TABLE_B0) == 0).all()
    worst = {}
    for (ref, kappa), t in zip(reference(bank, desc, RSIZE_B), T):
        assert (ref is None) == (t < 2)
        if ref is not None:
            assert np.isfinite(ref).all()
            worst[int(t)] = max(worst.get(int(t), 0.0), kappa)
    print("kappa by T:", {t: round(k, 1) for t, k in sorted(worst.items())})
    for t, cap in KAPPA_CAP.items():
        assert worst[t] <= cap, (t, worst[t])
    assert all(k <= 3.5 for t, k in worst.items() if t >= 31)


def test_table_e_covers_what_it_claims():
    _, desc = table_e()
    T = frames_of(desc[:, 1])
    assert len(T) == N_E > 1024 and set(T.tolist()) == {0, 5, 31, 33, 64, 65} and 15 <= (T == 0).sum() <= 25
    assert (desc[:, 1].max() <= 11000) and (desc[:, 0] + desc[:, 1] <= desc[-1, 0] + desc[-1, 1]).all()
    start, q, blocks = plan(T, G_MI355X)
    print("(e): %d tiles, q = %d" % (start[-1], q))
    assert 1300 <= start[-1] <= 1500 and q >= 2
    check_slots(T, G_MI355X)
    assert block_after_empty(T, G_MI355X) and any(len(runs) >= 3 for runs in blocks)
    assert T[1024] == 0 and T[1023] > 0 and T[1025] > 0           # thread 512 of the plan starts on a clip without a tile
