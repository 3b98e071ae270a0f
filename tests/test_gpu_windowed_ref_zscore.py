"""GPU: --get_reference_z_score in site windows (wgsassign_amd/zscore.py: reference_z_scores_windowed) held bit for bit to the resident
run on the same data (reference_z_scores, batch=4) and to the CPU restatement fed with the oracle's EM (tests/zscore_cpu.py): z, the
three sums, kept counts, the dictionary (keys, counts, means), AD_array, the iteration count of every masked fit and the printed
lines.  No tolerance anywhere.

The case is tests/test_gpu_windowed_zscore.py's, adapted: 20011 sites, windows of 8192 sites, so three windows with the last one ragged
(3627 sites); 8 individuals in populations of 3, 3 and 2, so every leave-one-out fit has 2, 2 or 1 members.  The inputs are
tests/synth_deep.py's (depth 1.5, jitter 0.01), with
  individual 2   every class of the depths 22 and 23 (kept deep depths), its deep sites on both sides of site 8192 and in window 3;
  individual 0   a class, (9, 3), whose only sites lie in window 2 and one, (3, 9), whose only sites lie in window 3;
  individual 5   no reads at all in window 2: it keeps nothing there and its chains hand their carries across that window.
The printed lines are compared with a resident run in its own blocks of 64 individuals (the order the command line prints in).
Every reference (the restatement, the resident runs) is computed once per option set and shared."""
import contextlib
import io

import numpy as np
import pytest

import synth
import synth_deep
import synth_depth
import zscore_cpu
from test_zscore_cpu import same

pytestmark = pytest.mark.gpu

M, N, K, W = 20011, 8, 3, 8192
ROLES, SIZES = ("none", "dropped", "kept", "single", "dropped", "none", "none", "dropped"), (3, 3, 2)
LATE = {(9, 3): (9000, 9001, 12345), (3, 9): (17000, 20000)}        # individual 0: classes that first appear in window 2 / window 3
TOLE = 1e-4
SHORT_ITER = 16             # a --maf_iter between the stopping iterations of the case's fits (test_some_fits_exhausted asserts that)
_case, _want, _resident, _files = [], {}, {}, {}


def case():
    if not _case:
        L, AD, IDs, A, deep = synth_deep.make_deep(M, N, K, 11, ROLES, sizes=SIZES)
        AD[W:2 * W, 10:12] = 0                                           # individual 5 has no reads in window 2
        for (Ar, Aa), sites in LATE.items():
            g0, g1 = synth_deep.class_triple(Ar, Aa)
            for s in sites:
                AD[s, 0:2] = (Ar, Aa)
                L[s, 0:2] = np.round(g0, 6), np.round(g1, 6)
        for a in (L, AD, A):
            a.setflags(write=False)
        _case.append((L, AD, IDs, A, deep))
    return _case[0]


def groups_of(IDs):
    pops = np.unique(IDs[:, 1])
    return np.searchsorted(pops, IDs[:, 1]).astype(np.int32), len(pops)


def restatement(oracle, thr=0, srt=False, lo=None, hi=None, maf_iter=200):
    key = (thr, srt, lo, hi, maf_iter)
    if key not in _want:
        L, AD, IDs, A, _ = case()
        _want[key] = zscore_cpu.reference(L, AD, IDs, lambda Lp, it, tol: oracle.emMAF(Lp, it, tol, 8), maf_iter, TOLE, thr, srt, lo, hi)
    return _want[key]


def resident_run(L, AD, IDs, thr=0, srt=False, lo=0, hi=None, maf_iter=200, batch=4):
    from wgsassign_amd import zscore
    from wgsassign_amd.device import DeviceBeagle
    group_of, n_groups = groups_of(IDs)
    b = DeviceBeagle.from_host(L, group_of, n_groups)
    depth = zscore.DepthTable(b, AD)
    details, lines = [], []
    try:
        z = zscore.reference_z_scores(b, depth, IDs, group_of, maf_iter, TOLE, thr, srt, lo, hi, batch=batch, say=lines.append, details=details)
    finally:
        depth.close()
        b.close()
    return z, details, lines


def resident(thr=0, srt=False, lo=0, hi=None, maf_iter=200):
    """The resident run's (z, details) in batches of 4 and its lines in its own blocks of 64, once per option set."""
    key = (thr, srt, lo, hi, maf_iter)
    if key not in _resident:
        L, AD, IDs, A, _ = case()
        z, details, _ = resident_run(L, AD, IDs, thr, srt, lo, hi, maf_iter, batch=4)
        z64, _, lines = resident_run(L, AD, IDs, thr, srt, lo, hi, maf_iter, batch=64)
        assert z64.tobytes() == z.tobytes()
        _resident[key] = (z, details, lines)
    return _resident[key]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    """The case's files, written once: Beagle (gzip), IDs, names, and the depth table as text, BGZF and .npy."""
    if not _files:
        L, AD, IDs, A, _ = case()
        d = tmp_path_factory.mktemp("zrefwin")
        p = synth_depth.write_inputs(str(d / "in"), L, AD, IDs, A)
        text = open(p["ad"], "rb").read()
        p["ad_bgzf"] = str(d / "in.ad.bgzf.gz")
        synth.write_bgzf(p["ad_bgzf"], text, block=20000)
        p["ad_npy"] = str(d / "in.ad.npy")
        np.save(p["ad_npy"], AD)
        _files.update(p)
    return _files


def windowed(paths, depth="ad", thr=0, srt=False, lo=0, hi=None, maf_iter=200, window_sites=W, IDs=None, group_of=None, **kw):
    from wgsassign_amd import zscore
    if IDs is None:
        IDs = case()[2]
    if group_of is None:
        group_of = groups_of(IDs)[0]
    details, lines = [], []
    z = zscore.reference_z_scores_windowed(paths["beagle"], paths[depth], IDs, group_of, maf_iter, TOLE, thr, srt, lo, hi,
                                           window_sites=window_sites, say=lines.append, details=details, **kw)
    return z, details, lines, dict(zscore.reference_z_scores_windowed.stats)


def compare(oracle, got, thr=0, srt=False, lo=0, hi=None, maf_iter=200):
    z, details, lines, stats = got
    rz, rdetails, rlines = resident(thr, srt, lo, hi, maf_iter)
    want = restatement(oracle, thr, srt, lo or None, hi, maf_iter)
    assert len(details) == len(rdetails) == len(want) > 0
    assert z.dtype == rz.dtype and z.tobytes() == rz.tobytes()
    assert lines == rlines
    for i, (d, r, w) in enumerate(zip(details, rdetails, want)):
        tag = "individual %d " % (lo + i)
        for k in ("keys", "counts", "means", "AD_array", "fac", "like", "index"):
            same(d[k], r[k], tag + k + " (resident)")
            same(d[k], w[k], tag + k + " (restatement)")
        assert d["kept"] == len(r["keep"]) == len(w["keep"]), tag + "kept"
        assert d["it"] == r["it"] == w["extra"], tag + "iteration of the masked fit"
        for k in ("W_l_obs", "z_mu", "z_var", "z"):
            same(np.float32(d[k]), np.float32(r[k]), tag + k + " (resident)")
            same(np.float32(d[k]), np.float32(w[k]), tag + k + " (restatement)")
        assert not {"keep", "wobs", "wl", "var", "A"} & set(d), tag + "a per-site array"
    assert zscore_cpu.file_text(z[:, 0]) == zscore_cpu.file_text([w["z"] for w in want])


def test_the_case_is_what_it_claims(oracle):
    """Conditions on the inputs, checked on the restatement."""
    L, AD, IDs, A, deep = case()
    want = restatement(oracle)
    group_of, n_groups = groups_of(IDs)
    assert n_groups == 3 and list(np.bincount(group_of)) == [3, 3, 2] and (M + W - 1) // W == 3 and M % W
    kept = [len(w["keep"]) for w in want]
    assert all(0.30 * M <= k <= 0.75 * M for j, k in enumerate(kept) if j != 5), kept
    assert 0.30 * (M - W) <= kept[5] <= 0.75 * (M - W), kept
    assert max(kept) > W
    per_window = [[int(((w["keep"] >= lo) & (w["keep"] < lo + W)).sum()) for lo in (0, W, 2 * W)] for w in want]
    assert per_window[5][1] == 0 and per_window[5][0] > 0 and per_window[5][2] > 0
    for (Ar, Aa), sites in LATE.items():
        where = np.flatnonzero((AD[:, 0] == Ar) & (AD[:, 1] == Aa))
        assert list(where) == list(sites)
        assert any((k == (Ar, Aa)).all() for k in want[0]["keys"])
    assert all(W <= s < 2 * W for s in LATE[(9, 3)]) and all(2 * W <= s for s in LATE[(3, 9)])
    assert sorted(set(int(d) for d in want[2]["AD_array"][:, 2] if d > 21)) == [22, 23]
    in_keep = deep[2][np.isin(deep[2], want[2]["keep"])]
    assert (in_keep < W).any() and ((in_keep >= W) & (in_keep < 2 * W)).any() and (in_keep >= 2 * W).any()
    iters = [w["extra"] for w in want]
    assert all(iters) and len(set(iters)) > 1, iters               # every fit converges inside 200 iterations, not all at the same one


def test_three_windows(oracle, paths):
    got = windowed(paths, depth_chunk_bytes=65536)             # (chunks of the depth file straddle both window edges)
    compare(oracle, got)
    stats = got[3]
    assert stats["windows"] == 3 and stats["window_sites"] == W and stats["rounds"] == 1 and stats["first_horizon"] == 32
    assert stats["fit_rounds"] == [len(stats["horizons"][0])] and stats["passes"] == 1 + stats["fit_rounds"][0] + 1
    assert len(stats["seconds_a"]) == 1 and len(stats["seconds_fit"][0]) == stats["fit_rounds"][0] and len(stats["seconds_final"][0]) == 1
    for one in [stats["depth_a"][0]] + stats["depth_fit"][0] + stats["depth_final"][0]:       # the depth file is read once per pass
        assert one["lines"] == M and one["chunks"] > 6
    # nothing of a window's size crosses: per pass the class sweep's tables or the carries, the open chunks at the end, the deep sites
    assert 0 < stats["downloaded_bytes"] <= N * (3 * 8191 * 4 + 3 * 4 + 3 * (253 * 20 + 4)) + 3 * 400 * 20 + stats["passes"] * 200 * N * 4


def test_threshold(oracle, paths):
    compare(oracle, windowed(paths, thr=3), thr=3)


def test_single_read_threshold(oracle, paths):
    compare(oracle, windowed(paths, srt=True), srt=True)


def test_individuals_inside_the_range(oracle, paths):
    compare(oracle, windowed(paths, lo=1, hi=7), lo=1, hi=7)


def test_rounds_of_individuals(oracle, paths):
    got = windowed(paths, batch=3)
    assert got[3]["rounds"] == 3 and got[2][0].startswith("wgsassign_amd: the z-scores of 8 individuals run in 3 rounds")
    assert len(got[3]["fit_rounds"]) == 3 and len(got[3]["seconds_a"]) == 3
    compare(oracle, (got[0], got[1], got[2][1:], got[3]))


def test_one_window(oracle, paths):
    got = windowed(paths, window_sites=24576)
    assert got[3]["windows"] == 1
    compare(oracle, got)


def test_first_horizon_of_all_iterations_takes_one_fit_round(oracle, paths):
    got = windowed(paths, first_horizon=200)
    assert got[3]["fit_rounds"] == [1] and got[3]["horizons"] == [[200]] and got[3]["passes"] == 3
    compare(oracle, got)


def test_first_horizon_of_two_takes_more_fit_rounds(oracle, paths):
    got = windowed(paths, first_horizon=2)
    assert got[3]["fit_rounds"][0] >= 2 and got[3]["horizons"][0][:2] == [2, 4] and got[3]["passes"] == got[3]["fit_rounds"][0] + 2
    compare(oracle, got)


def test_some_fits_exhausted(oracle, paths):
    """--maf_iter 16: in the resident run some fits stop by then and some do not (a condition on the input, asserted first); the
    exhausted ones report iteration 0, print nothing and take the frequencies of iteration 16."""
    rz, rdetails, rlines = resident(maf_iter=SHORT_ITER)
    its = [d["it"] for d in rdetails]
    assert 0 in its and any(its), its
    assert sum(ln.startswith("EM (MAF) converged") for ln in rlines) == sum(1 for t in its if t)
    got = windowed(paths, maf_iter=SHORT_ITER, first_horizon=5)
    assert got[3]["horizons"][0] == [5, 10, 16]
    compare(oracle, got, maf_iter=SHORT_ITER)


@pytest.mark.parametrize("depth", ["ad_bgzf", "ad_npy"])
def test_depth_file_formats(oracle, paths, depth):
    compare(oracle, windowed(paths, depth=depth, depth_chunk_bytes=65536))


def test_a_population_of_one_is_refused_before_the_first_pass(paths):
    from wgsassign_amd import zscore
    group_of = groups_of(case()[2])[0].copy()
    group_of[7] = 3                                             # individuals 6 and 7 are alone now
    zscore.reference_z_scores_windowed.stats = None
    with pytest.raises(ValueError, match="a population with a single individual has nobody left for the leave-one-out fit"):
        windowed(paths, group_of=group_of)
    assert zscore.reference_z_scores_windowed.stats is None
    got = windowed(paths, group_of=group_of, hi=6)              # ... but not when the range leaves them out
    assert len(got[1]) == 6


def test_an_individual_that_keeps_no_site(tmp_path):
    """Individual 7 has the two classes of depth 1, and in each of them likelihoods of 0.6 and 0.8: both survive the key filter, no
    site lies within 0.01 of its class mean.  The message is the one the resident run gives (wgs_em_fit_masked), after the first fit
    round."""
    from wgsassign_amd import zscore
    m = W + 1000
    L, AD, IDs, A, _ = case()
    L, AD = L[:m].copy(), AD[:m].copy()
    s = np.arange(m)
    AD[:, 14] = (s % 3 == 0)
    AD[:, 15] = (s % 3 == 1)
    L[:, 14] = np.where(s % 2 == 0, 0.6, 0.8).astype(np.float32)
    L[:, 15] = np.float32(0.1)
    with pytest.raises(ValueError) as resident_error:
        resident_run(L, AD, IDs, batch=64)
    assert str(resident_error.value) == "fit 7: no site was kept"
    p = synth_depth.write_inputs(str(tmp_path / "in"), L, AD, IDs, A[:m])
    with pytest.raises(ValueError) as windowed_error:
        windowed(p)
    assert str(windowed_error.value) == str(resident_error.value)
    lines = []
    with pytest.raises(ValueError, match="fit 4: no site was kept"):          # the fourth individual of the range from 3 on
        zscore.reference_z_scores_windowed(p["beagle"], p["ad"], IDs, groups_of(IDs)[0], 200, TOLE, ind_start=3, window_sites=W, say=lines.append)
    assert lines == []


def test_command_line(paths, tmp_path, monkeypatch, capfd):
    """WGSASSIGN_ZREF_WINDOW_SITES=8192 against the resident run of the same command: the bytes of .reference_z_ind.txt and the stdout
    lines; WGSASSIGN_Z_WINDOW_SITES alone leaves the run resident."""
    from wgsassign_amd import WGSassign
    runs = {}
    for tag, env in (("resident", None), ("other", "WGSASSIGN_Z_WINDOW_SITES"), ("windowed", "WGSASSIGN_ZREF_WINDOW_SITES")):
        out = str(tmp_path / tag)
        argv = ["--beagle", paths["beagle"], "--pop_af_IDs", paths["ids"], "--pop_names", paths["names"], "--ind_ad_file", paths["ad"],
                "--out", out, "--get_reference_z_score"]
        for name in ("WGSASSIGN_Z_WINDOW_SITES", "WGSASSIGN_ZREF_WINDOW_SITES"):
            monkeypatch.delenv(name, raising=False)
        if env:
            monkeypatch.setenv(env, str(W))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            WGSassign.main(argv)
        err = capfd.readouterr().err
        runs[tag] = (open(out + ".reference_z_ind.txt", "rb").read(), buf.getvalue().replace(out, "OUT").splitlines(), err)
    assert runs["windowed"][0] == runs["resident"][0] == runs["other"][0]
    assert runs["windowed"][1] == runs["resident"][1] == runs["other"][1]
    assert any(ln.startswith("EM (MAF) converged at iteration: ") for ln in runs["resident"][1])
    assert "reference z-scores in 1 rounds of individuals, " in runs["windowed"][2] and "passes over 3 windows of 8192 sites" in runs["windowed"][2]
    assert "reference z-scores in" not in runs["resident"][2] and "reference z-scores in" not in runs["other"][2]
    assert runs["resident"][0].decode() == zscore_cpu.file_text(resident()[0][:, 0])


# ---------------------------------------------------------------- the stream alone
T_STREAM = 16


def serial_chain(carry, a, b):
    d = a - b
    return np.cumsum(np.concatenate(([np.float32(carry)], d * d)).astype(np.float32), dtype=np.float32)[-1]


class TwoWindows:
    """12000 sites of the case as one joined matrix and as two windows fed from host matrices, with the case's dictionary (formed on
    the joined matrix) behind every kept-site set.  Individual 4 has no reads in the first window, individual 5 none in the second:
    each keeps nothing there.  want[t - 1][j]: the carry of iteration t of fit j over the joined matrix, formed on the host from the
    frequencies of the joined batch's own steps; iters: what wgs_em_fit_masked decides there."""

    def __init__(self):
        from wgsassign_amd import _lib, zscore
        from wgsassign_amd._lib import check, i32p
        from wgsassign_amd.device import DeviceBeagle, EMBatch, EMStream, chain_diff
        L, AD, IDs, A, _ = case()
        self.m = m = 12000
        L, AD = np.ascontiguousarray(L[:m]), AD[:m].copy()
        AD[:W, 8:10] = 0
        AD[W:, 10:12] = 0
        self.group_of, n_groups = groups_of(IDs)
        self.ids = np.arange(N, dtype=np.int32)
        self.sizes = np.bincount(self.group_of)
        joined = DeviceBeagle.from_host(L, self.group_of, n_groups)
        depth = zscore.DepthTable(joined, AD)
        summ = zscore.AD_summary(depth, 0, N, 0, False, True)
        self.tables = zscore.mask_tables(summ) + zscore.deep_tables(summ)
        keep = zscore.KeepSet(depth, 0, *self.tables)
        self.kept_total = keep.kept.copy()
        sites = [keep.sites(j) for j in range(N)]
        em = EMBatch(joined, self.group_of, self.ids)
        self.want = np.zeros((T_STREAM, N), dtype=np.float32)
        cur = [em.get_f(j) for j in range(N)]
        for t in range(1, T_STREAM + 1):
            prev = cur
            em.step()
            cur = [em.get_f(j) for j in range(N)]
            for j in range(N):
                self.want[t - 1, j] = serial_chain(0, cur[j][sites[j]], prev[j][sites[j]])
        em.close()
        em = EMBatch(joined, self.group_of, self.ids)
        self.iters = np.zeros(N, dtype=np.int32)
        check(_lib.load().wgs_em_fit_masked(em.handle, keep.handle, i32p(self.ids), T_STREAM, TOLE, i32p(self.iters)))
        self.decided = [next((t for t in range(1, T_STREAM + 1) if chain_diff(self.want[t - 1, j], self.kept_total[j]) < TOLE), 0) for j in range(N)]
        for x in (em, keep, depth, joined):
            x.close()
        self.windows = []
        for lo, hi in ((0, W), (W, m)):
            b = DeviceBeagle.from_host(np.ascontiguousarray(L[lo:hi]), self.group_of, n_groups, site0=lo)
            d = zscore.DepthTable(b, AD[lo:hi])
            k = zscore.KeepSet(d, 0, *self.tables)
            self.windows.append((b, d, k, EMBatch(b, self.group_of, self.ids)))
        self.stream = EMStream(N, T_STREAM, m)
        self.all_chains = [(j, t) for t in range(1, T_STREAM + 1) for j in range(N)]
        self.run = np.full(N, T_STREAM, dtype=np.int32)

    def push(self, w, chains=None, run=None, keep=None, em=None, slots=None, **kw):
        b, d, k, e = self.windows[w]
        self.stream.push_masked(em or e, keep or k, self.ids if slots is None else slots, self.run if run is None else run,
                                chains=self.all_chains if chains is None else chains, **kw)

    def close(self):
        self.stream.close()
        for b, d, k, e in self.windows:
            for x in (e, k, d, b):
                x.close()


@pytest.fixture(scope="module")
def two():
    t = TwoWindows()
    yield t
    t.close()


def test_stream_carries_are_those_of_the_joined_matrix(two):
    """Iteration for iteration: C after the two windows is the chain over the joined matrix's kept sites, and the first iteration at
    which it says converged is wgs_em_fit_masked's."""
    kept = [k.kept for _, _, k, _ in two.windows]
    assert kept[0][4] == 0 and kept[1][4] > 0 and kept[1][5] == 0 and kept[0][5] > 0      # a fit that keeps nothing in either window
    assert np.array_equal(kept[0] + kept[1], two.kept_total) and len(set(kept[0])) > 4
    assert list(two.iters) == two.decided and any(two.iters) and 0 in two.iters            # some fits stop inside 16 iterations, some do not
    two.push(0)
    two.push(1)
    C = two.stream.read_carries()
    assert C.tobytes() == two.want.tobytes()
    # a round that extends a horizon walks only the iterations above it: the carries below are not touched again (they start at 0)
    above = [(j, t) for j, t in two.all_chains if t > 6 and j != 3]
    two.push(0, chains=above)
    two.push(1, chains=above)
    C = two.stream.read_carries()
    assert C[6:, [0, 1, 2, 4, 5, 6, 7]].tobytes() == two.want[6:, [0, 1, 2, 4, 5, 6, 7]].tobytes()
    assert not C[:6].any() and not C[:, 3].any()


def test_final_fits_are_clamped_in_the_batch(two):
    """final: every fit run to its own stop and clamped with n_pop - 1 in the window's batch -- against the joined batch's frequencies."""
    from wgsassign_amd.device import DeviceBeagle, EMBatch
    L = case()[0][:two.m]
    stop = np.where(two.iters > 0, two.iters, T_STREAM).astype(np.int32)
    lo = (1 / (2 * two.sizes[two.group_of].astype(np.float64))).astype(np.float32)
    hi = (1 - 1 / (2 * two.sizes[two.group_of].astype(np.float64))).astype(np.float32)
    joined = DeviceBeagle.from_host(np.ascontiguousarray(L), two.group_of, 3)
    em = EMBatch(joined, two.group_of, two.ids)
    want = [None] * N
    for t in range(1, T_STREAM + 1):
        em.step()
        for j in range(N):
            if stop[j] == t:
                em.clamp(j, int(two.sizes[two.group_of[j]]) - 1)
                want[j] = em.get_f(j)
                em.set_active(j, False)
    em.close()
    joined.close()
    for w, (a, b) in enumerate(((0, W), (W, two.m))):
        two.push(w, chains=[], run=stop, final=np.ones(N, dtype=np.int32), clamp_lo=lo, clamp_hi=hi)
        for j in range(N):
            assert two.windows[w][3].get_f(j).tobytes() == want[j][a:b].tobytes(), (w, j)
    two.stream.read_carries()


def test_refusals_launch_nothing(two):
    """Every refusal is rc 2 (ValueError) with its message before any launch: the carries of the window pushed before are those the
    next good push goes on from."""
    from wgsassign_amd.device import EMBatch
    two.push(0)
    b1, d1, k1, e1 = two.windows[1]
    b0, d0, k0, e0 = two.windows[0]
    few = EMBatch(b1, two.group_of[:5], two.ids[:5])
    one = np.ones(N, dtype=np.int32)
    try:
        refused = [
            (dict(keep=k0), "the EM batch and the kept-site set belong to different matrices"),
            (dict(slots=np.array([0, 1, 2, 3, 4, 5, 6, 8], dtype=np.int32)), "fit 7: slot 8 outside the kept-site set"),
            (dict(slots=np.array([-1, 1, 2, 3, 4, 5, 6, 7], dtype=np.int32)), "fit 0: slot -1 outside the kept-site set"),
            (dict(run=np.array([T_STREAM - 1] + [T_STREAM] * 7, dtype=np.int32)), "iteration %d of fit 0, which runs %d" % (T_STREAM, T_STREAM - 1)),
            (dict(run=np.full(N, T_STREAM + 1, dtype=np.int32)), "fit 0: %d iterations, the fit stream has %d" % (T_STREAM + 1, T_STREAM)),
            (dict(chains=[(0, 5), (0, 4)]), "the chains are not sorted by iteration"),
            (dict(chains=[(8, 1)]), "chain 0: fit 8 out of range"),
            (dict(final=one), "final fits need their clamps"),
            (dict(em=e0, keep=k0), "but 8192 sites were pushed so far"),
        ]
        for kw, text in refused:
            with pytest.raises(ValueError) as e:
                two.push(1, **kw)
            assert text in str(e.value), (text, str(e.value))
        with pytest.raises(ValueError, match="the window's batch has 5 fits, the fit stream 8"):
            two.stream.push_masked(few, k1, two.ids, two.run, chains=[])
        with pytest.raises(ValueError, match="only 8192 of the 12000 sites were pushed"):
            two.stream.read_carries()
    finally:
        few.close()
    two.push(1)
    assert two.stream.read_carries().tobytes() == two.want.tobytes()
