"""The segment layout plan of a VO sequence (csrc/picp_vo_plan.cpp) on the CPU: bin/vo_plan, a
host-only program built with ASan/UBSan from that file alone, prints the plan of one case as JSON.

Every case is held to the invariants of the layout (the parts of the one allocation disjoint, on
256-B multiples, inside `total` and of the size their consumer indexes; the segment table's prefix
sums and map capacities; cap_c, npt; every frame->next problem once, in the first chunk that needs
it; one split count per launch vo_frame_match issues and scratch for each; each chain's scratch;
chains_eff), and to the decisions of the build before the plan was split out of the runtime:
tests/golden/vo_plan/plan_table.json was obtained by compiling that build's picp_vo_set_segments
planning code verbatim, with the same stand-ins for the matcher's two rules (the split rule with the
CU count as a parameter, the scratch rule as it stands), and running it on TABLE_CASES.  It holds
the scalars, ks_w, ks_p, chunk_off, every part's offset and `total`."""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, PKG

BIN = os.path.join(PKG, "bin", "vo_plan")
TABLE_FILE = os.path.join(GOLDEN, "vo_plan", "plan_table.json")
GRID_Y = 65535
PART_ORDER = ("segs", "boot", "mxyz", "mdesc", "mn", "planes", "probs", "stin", "stout", "wprobs", "lprobs", "eprobs",
              "pprobs", "poses", "steps", "pairs", "mh", "mn1", "mn2", "partw", "parte", "partp")
SCALARS = ("n_seg", "chains_eff", "max_steps", "npt", "map_slots", "n_slots", "max_map", "cap_c", "cap_p", "total")


def case(segs, obs, dim=10, chains=2, overlap=1, accept_only=1, split_env=0, early=None, ks_force=0, cus=256):
    """segs: (first, steps) pairs.  obs: per frame, a count or (repetitions, count).  early: the
    early streams exist (default: as picp_vo_create makes them, when split_env != 0)."""
    return dict(segs=[tuple(s) for s in segs], obs=list(obs), dim=dim, chains=chains, overlap=overlap,
                accept_only=accept_only, split_env=split_env, early=int(split_env != 0 if early is None else early),
                ks_force=ks_force, cus=cus)


def frame_sizes(c):
    out = []
    for o in c["obs"]:
        out += [o] if isinstance(o, int) else [o[1]] * o[0]
    return out


def segs_arg(segs):
    """first:steps pairs; a long run of equal steps at a constant stride as first:steps*count+stride
    (one argument holds at most 128 KiB)."""
    if len(segs) > 1000:
        (f0, st), stride = segs[0], segs[1][0] - segs[0][0]
        assert segs == [(f0 + k * stride, st) for k in range(len(segs))]
        return "%d:%d*%d+%d" % (f0, st, len(segs), stride)
    return ",".join("%d:%d" % s for s in segs)


def args_of(c):
    dp = 16 * (1 if c["dim"] <= 16 else 2)  # picp_match_prep_kch
    return [str(c[k]) for k in ("cus", "dim")] + [str(dp)] + [str(c[k]) for k in (
        "chains", "overlap", "accept_only", "split_env", "early", "ks_force")] + [
        segs_arg(c["segs"])] + [str(o) if isinstance(o, int) else "%dx%d" % o for o in c["obs"]]


def plan(c):
    r = subprocess.run([BIN] + args_of(c), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])  # the sanitizers report there
    return json.loads(r.stdout)


def scratch(ks, n, max_obs):
    """picp_match_split_scratch"""
    return ks * n * max_obs if ks > 1 else 0


def check_invariants(P, c):
    n = frame_sizes(c)
    first, steps = [s[0] for s in c["segs"]], [s[1] for s in c["segs"]]
    ns, dim, dp, max_obs = len(first), c["dim"], 16 * (1 if c["dim"] <= 16 else 2), max(n)
    assert P["n_seg"] == ns == len(P["segs"])
    # the segment table: prefix sums, capacities
    map_off = slot0 = 0
    caps = []
    for (f0, mo, s0, st), f, k in zip(P["segs"], first, steps):
        assert (f0, mo, s0, st) == (f, map_off, slot0, k)
        caps.append(n[f] + sum(n[f + t] for t in range(k)))
        map_off += max(caps[-1], 1)
        slot0 += k + 1
    assert (P["map_slots"], P["n_slots"], P["max_map"], P["max_steps"]) == (map_off, slot0, max(caps), max(steps))
    assert P["cap_c"] == (max(max_obs, 1) + 3) // 4 * 4
    assert P["npt"] == max([p for p in (1, 2, 4, 8) if p * 512 <= max_obs], default=1)
    # frame->next problems: every frame f0+k (k < steps) with observations exactly once, in the
    # first chunk that needs it
    want, chunk_off, seen = [], [0], set()
    off = [0]
    for z in n:
        off.append(off[-1] + z)
    for k in range(max(steps)):
        for f, st in zip(first, steps):
            if k < st and f + k not in seen and n[f + k] > 0:
                seen.add(f + k)
                want.append([off[f + k], n[f + k], off[f + k + 1], n[f + k + 1], 0])
        chunk_off.append(len(want))
    assert P["pprobs"] == want and P["chunk_off"] == chunk_off
    assert len(P["chunk_off"]) == P["max_steps"] + 1 and sorted(P["chunk_off"]) == P["chunk_off"]
    assert seen == {f + k for f, st in zip(first, steps) for k in range(st) if n[f + k] > 0}
    assert len({p[0] for p in want}) == len(want)
    # one split count at the start of every launch vo_frame_match issues; scratch for each
    nck = len(chunk_off) - 1
    spans = list(zip(chunk_off[:-1], chunk_off[1:])) if (c["overlap"] and nck > 1) else [(0, len(want))]
    launches = [(q, min(GRID_Y, p1 - q)) for p0, p1 in spans for q in range(p0, p1, GRID_Y)]
    assert [k[0] for k in P["ks_p"]] == [q for q, _ in launches]
    assert all(k[1] >= 1 for k in P["ks_p"])
    assert P["cap_p"] == max([scratch(k[1], m, max_obs) for k, (_, m) in zip(P["ks_p"], launches)], default=0)
    # chains: two groups never query one frame
    C = min(c["chains"], ns)
    group = lambda s: next(g for g in range(C) if s < ns * (g + 1) // C)
    q_group = {}
    for s, (f, st) in enumerate(zip(first, steps)):
        for t in range(st):
            q_group.setdefault(f + t + 1, set()).add(group(s))
    assert P["chains_eff"] == (1 if any(len(g) > 1 for g in q_group.values()) else C)
    C = P["chains_eff"]
    assert len(P["ks_w"]) == len(P["cap_w"]) == len(P["split_c"]) == len(P["cap_e"]) == C
    for ch in range(C):
        nsc = ns * (ch + 1) // C - ns * ch // C
        assert P["ks_w"][ch] >= 1 and P["cap_w"][ch] == scratch(P["ks_w"][ch], nsc, max_obs)
        assert P["split_c"][ch] == int(bool(c["early"]) and (c["split_env"] == 1 or (c["split_env"] < 0 and P["ks_w"][ch] > 1)))
        assert (P["cap_e"][ch] != 0) == bool(P["split_c"][ch])
        if P["split_c"][ch]:
            assert P["cap_e"][ch] == (P["ks_w"][ch] + 1) * nsc * max(max_obs, 1)
    # the one allocation: the size each consumer indexes, 256-B multiples, disjoint, inside total
    size = {"segs": ns * 32, "boot": ns * 32 * 4, "mxyz": map_off * 12, "mdesc": map_off * dim * 4, "mn": ns * 8,
            "planes": 5 * ns * P["cap_c"] * 4, "probs": ns * 24, "stin": ns * 128, "stout": ns * 128, "wprobs": ns * 40,
            "lprobs": ns * 40, "eprobs": 2 * ns * 40, "pprobs": max(len(want), 1) * 40, "poses": slot0 * 64,
            "steps": slot0 * 32, "pairs": ns * P["cap_c"] * 8, "mh": map_off * dp * 2, "mn1": map_off * 4,
            "mn2": map_off * 4, "partp": P["cap_p"] * 16}
    flat = []
    for name in PART_ORDER:
        if name in ("partw", "parte"):
            assert len(P["parts"][name]) == C
            for ch, p in enumerate(P["parts"][name]):
                assert p[1] == (P["cap_w"][ch] * 16 if name == "partw" else 2 * P["cap_e"][ch] * 16)
                flat.append(p)
        else:
            assert P["parts"][name][1] == size[name], name
            flat.append(P["parts"][name])
    at = 0
    for o, b in flat:  # in this order, each on the next 256-B multiple
        assert o % 256 == 0 and o == at, (o, at)
        at = o + (b + 255) // 256 * 256
    assert at == P["total"]


SEG3 = [(0, 4), (5, 3), (7, 4)]
LONG8 = [(80 * k, 80) for k in range(8)]  # four segments a chain, maps of 162,000 points
# the cases of the table (plan_table.json holds the earlier build's decisions for each, in order)
TABLE_CASES = [
    case([(0, 1)], [7, 9]),                                                  # two frames, one step
    case(SEG3, [300, 310, 0, 305, 290, 0, 300, 300, 300, 300, 300, 301]),    # empty frames: inside, and first
    case([(0, 3)], [1023] * 4), case([(0, 3)], [1024] * 4), case([(0, 3)], [1025] * 4),
    case([(0, 2)], [2047] * 3), case([(0, 2)], [2048] * 3),
    case([(0, 2)], [4095] * 3), case([(0, 2)], [4096] * 3), case([(0, 2)], [4097] * 3),
    case([(0, 4), (2, 4), (4, 4)], [(12, 601)]),                             # chains_eff drops to 1
    case([(0, 5)], [(6, 300)], chains=2),                                    # n_seg = 1
    case(SEG3, [(12, 300)], overlap=0, chains=1),
    case(SEG3, [(12, 300)], split_env=1),
    case(SEG3, [(12, 2000)], split_env=-1, dim=13),
    case(SEG3, [(12, 300)], ks_force=3),
    case([(k, 300) for k in range(300)], [(601, 1)], overlap=0),             # > 65,535 frame->next problems
    case(LONG8, [(641, 2000)]),                                              # a long-segment world match
]


def test_the_table_cases_match_the_earlier_build():
    with open(TABLE_FILE) as f:
        table = json.load(f)
    assert len(table) == len(TABLE_CASES)
    for c, want in zip(TABLE_CASES, table):
        P = plan(c)
        check_invariants(P, c)
        assert want["args"] == args_of(c)
        for k in SCALARS + ("ks_w", "ks_p", "chunk_off", "cap_w", "cap_e", "split_c"):
            assert P[k] == want[k], (c["segs"][:3], k)
        assert P["parts"] == want["parts"], c["segs"][:3]
        assert len(P["pprobs"]) == want["n_pprobs"]


def test_more_than_one_launch_of_frame_matches():
    """Overlap off, more than 65,535 frame->next problems: two launches, so two split counts.  A
    frame is matched once however many segments hold it (300 segments of 300 steps a frame apart
    are 599 problems: the table's case), so the problems here are two segments of 40,000 steps."""
    c = case([(0, 40000), (40000, 40000)], [(80001, 1)], overlap=0)
    P = plan(c)
    check_invariants(P, c)
    assert [k[0] for k in P["ks_p"]] == [0, GRID_Y] and len(P["pprobs"]) == 80000


@pytest.mark.parametrize("chains", [1, 2])
@pytest.mark.parametrize("overlap", [0, 1])
def test_invariants_over_schedules(chains, overlap):
    shapes = [
        ([(0, 1)], [7, 9]),
        (SEG3, [300, 310, 0, 305, 290, 0, 300, 300, 300, 300, 300, 301]),
        ([(0, 3)], [0, 5, 5, 5]),                        # a segment whose first frame is empty
        ([(0, 2), (1, 2)], [0, 0, 0, 0]),                # nothing anywhere
        ([(0, 3), (4, 2)], [1022, 1021, 7, 1022, 3, 1, 2]),  # max_obs no multiple of 4
        ([(0, 4), (2, 4), (4, 4)], [(12, 601)]),         # shared frames; two groups query frames 5, 6
        ([(0, 4), (1, 2), (3, 1)], [(6, 50)]),           # overlapping segments inside a group
        ([(0, 2), (3, 2), (6, 2)], [(9, 300)]),          # odd n_seg
        ([(0, 5)], [(6, 300)]),                          # n_seg = 1
    ]
    for segs, obs in shapes:
        for dim in (10, 12, 13):
            c = case(segs, obs, dim=dim, chains=chains, overlap=overlap)
            check_invariants(plan(c), c)


@pytest.mark.parametrize("max_obs,npt", [(1023, 1), (1024, 2), (1025, 2), (2047, 2), (2048, 4), (4095, 4), (4096, 8),
                                         (4097, 8), (511, 1), (12000, 8)])
def test_npt_steps(max_obs, npt):
    c = case([(0, 2)], [max_obs, 5, max_obs - 1])
    P = plan(c)
    check_invariants(P, c)
    assert P["npt"] == npt and P["cap_c"] % 4 == 0 and 0 <= P["cap_c"] - max_obs < 4


@pytest.mark.parametrize("split_env", [0, 1, -1])
@pytest.mark.parametrize("early", [0, 1])
def test_split_by_map_age(split_env, early):
    for obs in (300, 2000):
        for ks_force in (0, 1, 5):
            c = case(SEG3, [(12, obs)], split_env=split_env, early=early, ks_force=ks_force)
            P = plan(c)
            check_invariants(P, c)
            if ks_force:
                assert P["ks_w"] == [ks_force] * P["chains_eff"] and all(k[1] == ks_force for k in P["ks_p"])
            if not early or split_env == 0:
                assert not any(P["split_c"]) and not any(P["cap_e"])


def test_the_split_form_bit_flips_at_dim_12():
    """The folded accept-only form (dim <= 12) takes more ranges on a long-segment world match."""
    segs, obs = LONG8, [(641, 2000)]
    k12, k13 = (plan(case(segs, obs, dim=d))["ks_w"] for d in (12, 13))
    assert k12 == [32, 32] and k13 == [16, 16]
    assert plan(case(segs, obs, dim=12, accept_only=0))["ks_w"] == [16, 16]


def test_argument_errors_keep_their_messages():
    obs = [(12, 300)]
    assert plan(case([(0, 12)], obs))["error"] == \
        "picp_vo_set_segments: segment out of range (needs frames first .. first+steps, steps >= 1)"
    assert plan(case([(0, 0)], obs))["error"] == \
        "picp_vo_set_segments: segment out of range (needs frames first .. first+steps, steps >= 1)"
    assert plan(case([(0, 4), (5, 2), (5, 3)], obs))["error"] == \
        "picp_vo_set_segments: two segments start at frame 5 (they would query frame 6 at the same step)"
    assert plan(case([], obs))["error"] == "picp_vo_set_segments: n_seg must be in [1, 65535]"
    assert plan(case([(k, 1) for k in range(65536)], [(65538, 1)]))["error"] == \
        "picp_vo_set_segments: n_seg must be in [1, 65535]"
