"""The lane-parallel finish of a round (picp_solve6.h finish_round_lanes, the persistent kernel's)
against the uniform one (finish_round_pose, the graph path's round kernel): the same bits.

picp_selftest_finish runs both forms on the same totals, pose and loop state in one launch, one
wave per case, and counts the output words that differ: the twelve pose words, done, ok, converged,
chi_prev, chi_in, chi_out, n_in, n_projected.  The count must be 0.  The cases: a few thousand
systems from small seeded linearizations (the oracle's, at perturbed poses and several dampings),
and every input at which the finish takes another path -- the min-inlier early-out, a pivot at or
below FLT_MIN (the guarded solve), increment angles at the Taylor/libm threshold 0.0625 and one ulp
either side, one large angle with two small ones, NaN and Inf totals, the convergence rule with
conv_eps -1 and 1e-5 at chi_prev = FLT_MAX, chi_prev <= 1e-10 and a quotient equal to conv_eps, and
the last round (j == max_rounds).  Where the outcome is known in closed form the lane-parallel
form's own words are asserted too, so a selftest that compared nothing would not pass.

With H + damping I = I the solve returns dx = -b exactly (every product is by 1 or 0), which is how
the angle cases put an exact value into dx[3..5]."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234663852886e38)
FLT_MIN = np.float32(1.1754943508222875e-38)
THR = 3000.0
O_DONE, O_OK, O_CONV, O_CHI_PREV, O_CHI_IN, O_CHI_OUT, O_N_IN, O_N_PROJ = range(12, 20)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _ulp(x, k):
    return (np.array([x], np.float32).view(np.uint32) + np.uint32(k)).view(np.float32)[0] if k >= 0 else \
        (np.array([x], np.float32).view(np.uint32) - np.uint32(-k)).view(np.float32)[0]


def _pose_words(T):
    T = np.asarray(T, np.float32)
    return np.concatenate([T[:3, :3].T.reshape(9), T[:3, 3]])  # R column-major, t


def _case(H, b, pose, chi_in=10.0, chi_out=0.0, n_in=50, n_proj=60, damping=1.0, chi_prev=FLT_MAX,
          conv_eps=-1.0, min_inliers=0, max_rounds=50, j=3):
    """One input of picp_selftest_finish (include/picp_c.h): the totals as the kernels convert them
    (damping added in double, then float; -b)."""
    w = np.zeros(52, np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):  # the NaN/Inf cases
        Hd = np.asarray(H, np.float64) + float(damping) * np.eye(6)
        w[:21] = _bits([Hd[r, c] for r in range(6) for c in range(r, 6)])
        w[21:27] = _bits(-np.asarray(b, np.float64))
    w[27], w[28] = _bits(chi_in), _bits(chi_out)
    w[29:31] = np.array([n_in, n_proj], np.int32).view(np.uint32)
    w[32:44] = _bits(pose)
    w[44], w[45] = _bits(chi_prev), _bits(conv_eps)
    w[46:49] = np.array([min_inliers, max_rounds, j], np.int32).view(np.uint32)
    return w


def _dx_case(dx, pose, **kw):
    """H + damping I = I and -b = dx: the solve returns dx exactly."""
    return _case(np.zeros((6, 6)), -np.asarray(dx, np.float64), pose, damping=1.0, **kw)


@pytest.fixture(scope="module")
def seeded(oracle):
    """(cases, n) from 256 frames of 64 correspondences, each linearized once and used at eight
    (damping, pose, loop state) combinations."""
    from picp_amd import synth
    rng = np.random.default_rng(20250101)
    out = []
    for s in range(256):
        p = synth.make_problem(64, seed=9000 + s, outlier_frac=0.2, pixel_noise=0.5)
        lin = oracle.linearize(p["T_init"], p["K"], 480, 640, p["world"], p["image"], p["pairs"], THR,
                               mode=oracle.MODE_F64)
        for k in range(8):
            pose = _pose_words(p["T_init"])
            if k & 1:  # any twelve floats are a valid input: the update is three products per word
                pose = (pose * rng.uniform(0.5, 2.0, 12) * rng.choice([-1.0, 1.0], 12)).astype(np.float32)
            scale = 10.0 ** rng.uniform(-3, 1)  # larger increments: some angles pass 0.0625
            out.append(_case(lin["H"] * scale, lin["b"], pose, chi_in=lin["chi_in"], chi_out=lin["chi_out"],
                             n_in=lin["n_in"], n_proj=lin["n_projected"], damping=(1.0, 0.0, 100.0, 1e-3)[k >> 1],
                             chi_prev=(FLT_MAX, lin["chi_in"] * (1 + 10.0 ** rng.uniform(-7, -3)))[k & 1],
                             conv_eps=(-1.0, 1e-5)[(k >> 1) & 1], j=1 + (s + k) % 50))
    return np.stack(out)


def _edge_cases():
    from picp_amd import synth
    T = synth.make_problem(8, seed=1)["T_init"]
    pose = _pose_words(T)
    neg0 = np.full(12, -0.0, np.float32)
    H = np.diag([4.0, 3.0, 5.0, 6.0, 7.0, 8.0]) + 0.25
    b = np.array([0.1, -0.2, 0.3, 0.01, -0.02, 0.03])
    cases, expect = [], []  # expect: (index, {word: value}) of the lane-parallel form's outputs

    def add(c, **exp):
        if exp:
            expect.append((len(cases), exp))
        cases.append(c)

    # the min-inlier early-out: the pose stays, ok 0, done 1
    for n_in, mi in ((4, 5), (0, 1), (49, 50)):
        add(_case(H, b, pose, n_in=n_in, min_inliers=mi), pose=pose, ok=0, done=1, conv=0, n_in=n_in)
    add(_case(H, b, pose, n_in=50, min_inliers=50), ok=1, done=0)  # n_in == min_inliers solves
    # a pivot at or below FLT_MIN (1/d = 0): the first, a later one (4 - 2 * 2 / 1 = 0), a denormal
    for d0 in (0.0, float(FLT_MIN), float(FLT_MIN) / 2, -float(FLT_MIN), float(_ulp(FLT_MIN, 1))):
        Hs = H.copy()
        Hs[0, 0] = d0
        add(_case(Hs, b, pose, damping=0.0))
    Hs = H.copy()
    Hs[0, 0], Hs[0, 1], Hs[1, 0], Hs[1, 1] = 1.0, 2.0, 2.0, 4.0
    add(_case(Hs, b, pose, damping=0.0))
    add(_case(np.zeros((6, 6)), b, pose, damping=0.0))  # every pivot zero: dx = 0
    # the angles at the threshold and one ulp either side, each in every position and sign
    for a in (np.float32(0.0625), _ulp(0.0625, 1), _ulp(0.0625, -1)):
        for pos in range(3):
            for sgn in (1.0, -1.0):
                dx = np.array([0.1, -0.2, 0.3, 0.01, -0.02, 0.03], np.float32)
                dx[3 + pos] = sgn * a
                add(_dx_case(dx, pose))
        add(_dx_case([0.0, 0.0, 0.0, a, -a, a], pose))
    for pos in range(3):  # one large, two small
        for big in (1.0, -2.5, 100.0, 1e6):
            dx = np.array([0.1, -0.2, 0.3, 0.01, -0.02, 0.03], np.float32)
            dx[3 + pos] = big
            add(_dx_case(dx, pose))
    add(_dx_case(np.zeros(6), pose, j=7, max_rounds=50), pose=pose, ok=1, done=0)  # dx = 0: Rd = I, the pose stays
    add(_dx_case(np.zeros(6), neg0))                   # -0 words through the t select
    add(_dx_case([-0.0, -0.0, -0.0, 0.0, 0.0, 0.0], neg0))
    # NaN and Inf totals: in H, in b (a NaN angle takes the libm path), in chi
    for v in (np.nan, np.inf, -np.inf):
        Hs = H.copy()
        Hs[2, 2] = v
        add(_case(Hs, b, pose))
        for i in (0, 3, 4, 5):
            bs = b.copy()
            bs[i] = v
            add(_case(H, bs, pose))
        add(_case(H, b, pose, chi_in=v, conv_eps=1e-5, chi_prev=1.0))
        add(_case(H, b, pose, chi_in=1.0, conv_eps=1e-5, chi_prev=v))
        add(_case(H, b, pose, chi_out=v))
    # the convergence rule (exec/icp_test.cpp:99-106): rel = prev > 1e-10 ? |prev - cur| / prev : 0
    for eps in (-1.0, 1e-5):
        conv0 = 1 if eps > 0 else 0  # rel = 0 < 1e-5 converges; nothing is below -1
        add(_case(H, b, pose, chi_in=10.0, chi_prev=FLT_MAX, conv_eps=eps), conv=0, done=0, chi_prev=10.0)
        for prev in (1e-10, 5e-11, 0.0, -1.0):
            add(_case(H, b, pose, chi_in=10.0, chi_prev=prev, conv_eps=eps), conv=conv0, done=conv0,
                chi_prev=prev if conv0 else 10.0)
        add(_case(H, b, pose, chi_in=10.0, chi_prev=float(_ulp(1e-10, 1)), conv_eps=eps), conv=0, done=0)
        add(_case(H, b, pose, chi_in=10.0, chi_prev=10.0, conv_eps=eps), conv=conv0, done=conv0)
    # |prev - cur| / prev == 1e-5f exactly (checked below): not below conv_eps, so no convergence;
    # cur one ulp nearer to prev converges
    prev_q = np.array([0x3f802c80], np.uint32).view(np.float32)[0]
    cur_q = np.array([0x3f802c2c], np.uint32).view(np.float32)[0]
    assert np.float32(np.abs(prev_q - cur_q) / prev_q) == np.float32(1e-5)
    add(_case(H, b, pose, chi_in=cur_q, chi_prev=prev_q, conv_eps=1e-5), conv=0, done=0, chi_prev=cur_q)
    add(_case(H, b, pose, chi_in=_ulp(cur_q, 1), chi_prev=prev_q, conv_eps=1e-5), conv=1, done=1, chi_prev=prev_q)
    add(_case(H, b, pose, chi_in=_ulp(cur_q, -1), chi_prev=prev_q, conv_eps=1e-5), conv=0, done=0)
    # the last round
    add(_case(H, b, pose, j=50, max_rounds=50), done=1, conv=0, ok=1)
    add(_case(H, b, pose, j=49, max_rounds=50), done=0)
    add(_case(H, b, pose, j=1, max_rounds=1, chi_prev=10.0, conv_eps=1e-5), done=1, conv=1)
    return np.stack(cases), expect


def test_edge_inputs_same_bits_and_known_outcomes(native):
    cases, expect = _edge_cases()
    bad, out, ref = native.selftest_finish(cases)
    print("edge cases %d, differing words %d" % (len(cases), bad))
    for i, j in zip(*np.nonzero(out != ref)):
        print("  case %d word %d: lanes %08x uniform %08x" % (i, j, out[i, j], ref[i, j]))
    assert bad == 0
    key = {"done": O_DONE, "ok": O_OK, "conv": O_CONV, "n_in": O_N_IN}
    for i, exp in expect:
        for k, v in exp.items():
            if k == "pose":
                np.testing.assert_array_equal(out[i, :12], _bits(v), err_msg="case %d pose" % i)
            elif k == "chi_prev":
                assert out[i, O_CHI_PREV] == _bits(v), (i, k)
            else:
                assert int(out[i, key[k]]) == v, (i, k, int(out[i, key[k]]))
    # every case carries its statistics through unchanged
    np.testing.assert_array_equal(out[:, O_CHI_IN], cases[:, 27])
    np.testing.assert_array_equal(out[:, O_CHI_OUT], cases[:, 28])
    np.testing.assert_array_equal(out[:, O_N_IN:O_N_PROJ + 1], cases[:, 29:31])


def test_seeded_systems_same_bits(native, seeded):
    bad, out, ref = native.selftest_finish(seeded)
    print("seeded cases %d, differing words %d" % (len(seeded), bad))
    assert bad == np.count_nonzero(out != ref)
    assert len(seeded) >= 2000
    assert bad == 0
    # the update moved the pose (the selftest did run the solve) and stayed finite
    moved = (out[:, :12] != seeded[:, 32:44]).any(axis=1)
    assert moved.mean() > 0.99
    assert np.isfinite(out[:, :12].view(np.float32)).all()


def test_update_matches_float_reference(native, oracle):
    """The new pose against v2tEuler(dx) * T computed here in float64 from the exact dx of
    identity systems: the selftest's two forms agreeing with each other is not the only anchor."""
    from picp_amd import synth
    rng = np.random.default_rng(7)
    T = synth.make_problem(8, seed=2)["T_init"].astype(np.float64)
    dxs = np.concatenate([rng.uniform(-0.05, 0.05, (32, 6)), rng.uniform(-1.5, 1.5, (32, 6))]).astype(np.float32)
    cases = np.stack([_dx_case(dx, _pose_words(T)) for dx in dxs])
    bad, out, ref = native.selftest_finish(cases)
    assert bad == 0
    for dx, o in zip(dxs, out):
        D = np.eye(4)
        D[:3, :3] = synth.euler_xyz(*dx[3:].astype(np.float64))
        D[:3, 3] = dx[:3]
        ref = D @ np.asarray(np.float32(T), np.float64)
        got = o[:12].view(np.float32)
        # float32 products of O(1) entries (|t| < 8 here): a few ulps of the largest term
        np.testing.assert_allclose(got[:9].reshape(3, 3).T, ref[:3, :3], atol=4e-6)
        np.testing.assert_allclose(got[9:], ref[:3, 3], atol=4e-6 * max(1.0, np.abs(ref[:3, 3]).max()))
