"""-m gpu: npa_world_behave (csrc/behave.hip) on the inputs tests/test_behave_gpu.py leaves out.

* behave_cases.EDGES, literals bit for bit: rows that are no agent, a null array with stride 0, seg_limit 0, the counter's wrap,
  the branches of the arithmetic no other decided case takes;
* behave_cases.RANDOM_EDGES against the restatement (tests/behave_ref.py) under the rule of test_behave_gpu.py -- equal index
  wherever the restatement's two lowest costs differ by more than 1e-12 relative, here with no agent left out; goals, counters and
  velocities bitwise; poisoned rows and guards: the candidate cap (eight trips), three and four chunks of discs, a chunk boundary
  inside the robots, seg_limit inside a chunk of capsules, two commit workgroups per world, an infinite horizon, worlds of a batch
  with counts of 0.  tests/test_behave.py shows on the restatement that each result hangs on the chunk, trip or horizon it is for;
* counts outside their strides, which both kernels clamp;
* the generator where its 64-bit sum wraps and where the counter and the world index use bit 31."""
import numpy as np
import pytest

import behave_cases as bc
import behave_ref as ref
from test_behave_gpu import check_decided, compare, device_behave

pytestmark = pytest.mark.gpu


def same_bits(a, b, what):
    for g, h in zip(a, b):
        for k in g:
            assert g[k].tobytes() == h[k].tobytes(), (what, k)


# ---------------------------------------------------------------------------------------------------- decided cases
@pytest.mark.parametrize("case", bc.EDGES, ids=lambda c: c["name"])
def test_edges(case):
    """the literals of behave_cases.EDGES, bit for bit.
    item 1, no_agent_*: a row with first < 0, count < 1, a circle with count != 1, first = nC + nS or a run past n_segments is
      bitwise its input in all ten columns and in `draws`, is nobody's neighbour (row 0 meets circle 1 as a plain circle) and owns
      nothing (circle 1's velocity columns stay); the control with one valid segment does move;
    item 3, segments_only / circles_only: run padded, then with the absent array a null pointer and its stride 0 -- the same bits;
    item 6, seg_limit_zero: every segment hidden;
    item 7, draws_wrap: the int32 -1 is draw number 4294967295, the counter wraps to 0, the second call draws number 0;
    item 9: vcur_clamped (candidate 2 scaled to v_max wins), point_segment_* (e2 == 0: one disc, both shifted segments invalid),
      moving_wall_* (a segment's velocity is the capsule's apex), L0_threshold_negative (L == 0 rests, nothing drawn) and
      L0_threshold_zero (L == 0 is arrived at threshold 0: a redraw)."""
    got = device_behave(case)
    check_decided(case, got, case["expect"])
    if case["null"]:
        for k in case["null"]:
            assert all(len(wd[k]) == 0 for wd in case["worlds"])
        bare = device_behave(case, pad={k: 0 for k in case["null"]})
        check_decided(case, bare, case["expect"])
        same_bits(bare, got, case["name"])
    if case["expect2"] is not None:
        check_decided(case, device_behave(case, calls=2), case["expect2"])


# ---------------------------------------------------------------------------------------------------- random worlds
@pytest.mark.parametrize("spec", bc.RANDOM_EDGES, ids=lambda s: s[0])
def test_random_edges_against_the_restatement(spec):
    """item 4, commit2blk: strides 255 + 30 = 285 primitives: commit workgroups 0 and 1 of world 0, 2 and 3 of world 1; workgroup 1
      holds segments only (rows 1 - 29), the owned rows 20 - 27 among them;
    item 5, c512: 512 candidates = the cap = trips 0 - 7 (the restatement chooses in trips 6 and 7); c192: three full trips;
    item 6: d200: 199 discs in chunks of 64, 64, 64, 7; r70 / r70_noprev: 81 discs, robots 53 - 69 in chunk 1, with and without
      prev_state; s148_lim100 / s148_lim0 / s148_open: 148 segments, seg_limit inside chunk 1, 0, and none (three chunks), the
      polygon agents' edges 140 - 147 beyond the cut; hz_inf: horizon = +inf keeps every neighbour; ragged: three worlds under common
      strides with 0 agents, 0 circles, 0 segments.
    No agent may be left out: every choice of these seeds is decided (tests/test_behave.py)."""
    case = bc.random_case(spec)
    res = ref.run_case(case)
    got = device_behave(case)
    agents, left = compare(case, got, res)
    print(spec[0], "agents", agents, "left out", left, "chosen", [o["chosen"].tolist() for o in res])
    assert left == 0 and agents == sum(len(wd["rows"]) for wd in case["worlds"])
    same_bits(device_behave(case), got, spec[0])                 # the call is a function of its inputs


def test_ragged_worlds_alone_and_in_the_batch():
    """item 6, per-world counts of 0 beside others: each world of `ragged` alone (its own strides, world_base = w) gives the bits it
    gives in the batch; the world without agents comes back as it went in"""
    case = bc.random_case([s for s in bc.RANDOM_EDGES if s[0] == "ragged"][0])
    got = device_behave(case)
    for w, wd in enumerate(case["worlds"]):
        one = dict(case, worlds=[wd], robots=case["robots"][w:w + 1], prev=case["prev"][w:w + 1])
        same_bits(device_behave(one, world_base=w), got[w:w + 1], w)
    for k in ("circles", "segments"):
        assert got[0][k].tobytes() == case["worlds"][0][k].tobytes()


# ---------------------------------------------------------------------------------------------------- counts outside the strides
def _count_case():
    case = bc.random_case(bc.RANDOM[4])                          # one world: 5 agents (2 squares), 10 circles, 17 segments, 3 robots
    wd = case["worlds"][0]
    return case, wd, (len(wd["circles"]), len(wd["segments"]), len(wd["rows"]))


def _restated(case, wd, counts, segments=None):
    o = ref.behave_world(wd["circles"], wd["segments"] if segments is None else segments, wd["rows"], wd["idx"], case["par"], case["robots"],
                         case["prev"], case["radius"], case["seg_limit"], case["dirs"], case["n_speed"], case["dt"], counts=counts)
    assert all(c is None or ref.decided(c) for c in o["costs"])
    return o


def _bitwise(got, o, keys=("circles", "segments", "rows", "idx")):
    for k in keys:
        want = o[k].astype(np.int32) if k == "idx" else o[k]
        assert got[k].tobytes() == want.tobytes(), k


@pytest.mark.parametrize("which", ["agents_over", "agents_negative", "circles_over", "segments_negative"])
def test_counts_outside_their_strides(which):
    """item 2: n_agents, n_circles and n_segments are clamped to [0, stride] in both kernels; the tables are full to their strides
    (pad 0) where a count exceeds them, so every row the clamped count admits is valid.  Bitwise against the restatement fed the
    same counts; the count arrays come back unchanged (device_behave).
      n_agents = a_stride + 7: all a_stride rows act;  n_agents = -3: every table comes back as it went in;
      n_circles = c_stride + 5: as c_stride;  n_segments = -2: the polygon rows are no agents (item 1), no segment is a neighbour,
      none is written, and the circle agents choose as in the world without segments."""
    case, wd, (nC, nS, nA) = _count_case()
    plain = _restated(case, wd, None)
    if which == "agents_over":
        got = device_behave(case, pad=dict(rows=0), counts=dict(rows=[nA + 7]))[0]
        _bitwise(got, _restated(case, wd, (nC, nS, nA + 7)))
        _bitwise(got, plain)
    elif which == "agents_negative":
        got = device_behave(case, counts=dict(rows=[-3]))[0]
        _bitwise(got, _restated(case, wd, (nC, nS, -3)))
        for k in ("circles", "segments", "rows", "idx"):
            assert got[k].tobytes() == wd[k].tobytes(), k
    elif which == "circles_over":
        got = device_behave(case, pad=dict(circles=0), counts=dict(circles=[nC + 5]))[0]
        _bitwise(got, _restated(case, wd, (nC + 5, nS, nA)))
        _bitwise(got, plain)
    else:
        got = device_behave(case, counts=dict(segments=[-2]))[0]
        o = _restated(case, wd, (nC, -2, nA))
        _bitwise(got, o)
        assert got["segments"].tobytes() == wd["segments"].tobytes()
        bare = _restated(case, wd, None, segments=np.zeros((0, 6)))                 # the world without segments
        _bitwise(got, bare, keys=("circles", "rows", "idx"))
        polygon = wd["idx"][:, 0] >= nC
        assert polygon.sum() == 2 and got["rows"][polygon].tobytes() == wd["rows"][polygon].tobytes()
        assert (got["rows"][~polygon, 9] >= 0).all() and got["rows"].tobytes() != plain["rows"].tobytes()


# ---------------------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("seed,world_base", [((1 << 64) - 1, 1), ((1 << 64) - 5, (1 << 31) - 2), (2008, (1 << 31) - 2)])
def test_generator_where_the_sum_wraps(seed, world_base):
    """item 7 and item 8: 130 agents that stand at their goals draw from (seed, world_base + 0, first, draws) with the 64-bit sum
    seed + world wrapping, the world index at the largest value npa_world_behave accepts for one world, and the counter at
    2^31 - 1, 2^31 and 2^32 - 1 (int32 -2^31 and -1): the goals are those of the unsigned draw number, the counter + 1 mod 2^32,
    through the restatement's whole call and through draw_goal alone"""
    n = 130
    C_ = np.zeros((n, 6))
    C_[:, 0], C_[:, 1], C_[:, 2] = 64.0 * (np.arange(n) % 16), 64.0 * (np.arange(n) // 16), 0.5
    rows = np.array([bc.agent_row(C_[k, 0], C_[k, 1]) for k in range(n)])
    for draws in ((1 << 31) - 1, 1 << 31, (1 << 32) - 1):
        idx = np.array([[k, 1, 1, 0] for k in range(n)], dtype=np.int32)
        idx[:, 3] = np.uint32(draws).astype(np.int32)
        case = bc.case("generator", [bc.world(C_, (), rows, idx)], None, horizon=0.5, lo=(-3.0, 5.0), hi=(9.0, 5.5), seed=seed,
                       dirs=np.zeros((0, 2)), n_speed=0)
        got = device_behave(case, world_base=world_base)[0]
        want = np.array([ref.draw_goal(seed, world_base, k, draws, (-3.0, 5.0), (9.0, 5.5)) for k in range(n)])
        assert got["rows"][:, 0:2].tobytes() == want.tobytes()
        assert (got["idx"][:, 3].astype(np.uint32) == np.uint32((draws + 1) & 0xFFFFFFFF)).all()
        assert (got["rows"][:, 9] == 1).all()                    # everybody alone within the horizon: towards the new goal
        _bitwise(got, ref.run_case(case, world_base=world_base)[0])
