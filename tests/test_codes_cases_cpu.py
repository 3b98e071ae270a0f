"""CPU-only: tests/codes_cases.py held to its own claims -- the chains' keys share the stated home slot under the restated hash,
the stated class counts are those of the matrices, every case stands at every required lane position, the sample pass will code
every matrix, and a digest of each matrix is recorded so that a later change of the cases is visible."""
import numpy as np
import pytest

import codes_cases as cc
import synth

MATRIX_NAMES = ("chains_0", "chains_1", "chains_2", "chains_3", "chains_4", "chains_5", "chains_6", "limits_0", "limits_1", "edges_0",
                "edges_1", "groups")

DIGESTS = {
    (64, "chains_0"): "67586957fe6062e6",
    (64, "chains_1"): "4e33327c492cbea5",
    (64, "chains_2"): "6a5f4008880bbb3f",
    (64, "chains_3"): "4b798052d7646d8c",
    (64, "chains_4"): "03754fe7102bd197",
    (64, "chains_5"): "b4244a607a987953",
    (64, "chains_6"): "cb4910a05c792650",
    (64, "limits_0"): "d99717c79dbfc943",
    (64, "limits_1"): "9eca77ad7ec4a9c7",
    (64, "edges_0"): "fc8e416602f0cffb",
    (64, "edges_1"): "d0e7815b5e6a279b",
    (64, "groups"): "e285719d4e3bcab2",
    (128, "chains_0"): "a68785b81e044b82",
    (128, "chains_1"): "451cb443f774979a",
    (128, "chains_2"): "99942a7efaa2f641",
    (128, "chains_3"): "6ace1034bdcc2450",
    (128, "chains_4"): "8fb2cd5a8ee3a21b",
    (128, "chains_5"): "31ad3021ca66d069",
    (128, "chains_6"): "1af970d35a5165bd",
    (128, "limits_0"): "62a50ec12e290a63",
    (128, "limits_1"): "363ca21c1e1b406b",
    (128, "edges_0"): "365df8c136c82237",
    (128, "edges_1"): "7ddaa419c46717bd",
    (128, "groups"): "ffcb46d257562467",
    (256, "chains_0"): "dd0162f2b77b5650",
    (256, "chains_1"): "e35c7e2803d14b97",
    (256, "chains_2"): "abff548978331736",
    (256, "chains_3"): "c6d91b234f742041",
    (256, "chains_4"): "ac02cb9d1308055d",
    (256, "chains_5"): "d96521b68a2dd2a0",
    (256, "chains_6"): "cb920133b8e91889",
    (256, "limits_0"): "26eec6cea806cbb2",
    (256, "limits_1"): "660e0689fb899608",
    (256, "edges_0"): "84a3e0e8d1058ef8",
    (256, "edges_1"): "fd84dcd67432549d",
    (256, "groups"): "40e256a9c3535d8c",
}


ORDER_DIGESTS = {64: "ae2e817c120923ed", 128: "969598d4c3ab10ee", 256: "3a250948562737bb"}
SPARSE_DIGESTS = {64: "df67211e1653a810", 128: "8710d9c6dd313e68", 256: "2bb3a2028d6633ac"}


def scalar_hash(g0, g1):
    """hash32 of csrc/codes_kernels.hip on Python integers"""
    rot = lambda v, r: ((v << r) | (v >> (32 - r))) & 0xFFFFFFFF
    x = g0 ^ rot(g1, 13)
    return (((x & 0xFFFFFF) * 0x9E3779) & 0xFFFFFFFF) ^ rot((((x >> 8) & 0xFFFFFF) * 0x85EBCB) & 0xFFFFFFFF, 3)


def test_the_restated_hash():
    g0, g1, home = cc.key_pool()
    for i in range(0, len(g0), len(g0) // 500):
        h = scalar_hash(int(g0[i]), int(g1[i]))
        assert int(cc.hash32(g0[i:i + 1], g1[i:i + 1])[0]) == h
        for T, shift in ((64, 26), (128, 25), (256, 24)):
            assert int(cc.home_slot(g0[i:i + 1], g1[i:i + 1], T)[0]) == h >> shift
        assert home[i] == h >> 24
    assert scalar_hash(0xFFFFFFFF, 0xFFFFFFFF) == 0                # KEY_EMPTY's own home is slot 0
    # what a Beagle file can hold: six decimals, g0 + g1 <= 1
    v0, v1 = g0.view(np.float32).astype(np.float64), g1.view(np.float32).astype(np.float64)
    assert np.array_equal(np.round(v0, 6).astype(np.float32).view(np.uint32), g0) and (v0 + v1 <= 1.0 + 1e-6).all() and (v0 >= 0).all()


@pytest.mark.parametrize("T", cc.GEOMETRIES)
def test_cases_keep_their_claims(T):
    G = cc.Geometry(T)
    mats = cc.build(T)
    assert tuple(M.name for M in mats) == MATRIX_NAMES
    assert (G.snps, G.cols, G.buffer) == {64: (16, 4, 32), 128: (8, 8, 64), 256: (4, 16, 128)}[T]
    seen_cases = set()
    for M in mats:
        assert M.L.shape == (M.m, 2 * G.n) and M.m % 64 != 0 and 400 <= M.m <= 4400 and G.n >= 257
        assert np.array_equal(M.counts, synth.classes_per_snp(M.L))
        Lb = M.L.view(np.uint32)
        g0, g1 = Lb[:, 0::2], Lb[:, 1::2]
        empty = (g0 == cc.KEY_EMPTY_WORD) & (g1 == cc.KEY_EMPTY_WORD)
        assert np.array_equal(empty.any(axis=1), M.names == "bits_key_empty")
        for g, size in enumerate(G.slab_sizes):
            a, b = cc.slab_range(G, g)
            assert (M.labels[a:b] == g).all() and b - a == size
            if size:
                assert np.array_equal(M.slab_counts[:, g], synth.classes_per_snp(M.L[:, 2 * a:2 * b]))
        assert (M.slab_counts.max(axis=1) <= M.counts).all() and (M.slab_counts[:, cc.EMPTY_SLAB] == 0).all()
        home = cc.home_slot(g0, g1, T)
        for i in range(M.m):
            f = M.facts[i]
            if "count" in f:
                assert M.counts[i] == f["count"], (M.name, M.names[i])
            if "chain" in f:
                assert M.counts[i] == f["chain"] and (home[i] == f["home"]).all(), (M.name, M.names[i])
                assert M.expect[i] == ("coded" if f["chain"] <= cc.ENC_RMAX else "either")
                if f["spread"] == "buffer":                      # all of the chain within the first min(c, buffer) individuals
                    k = min(f["chain"], G.buffer)
                    assert len(set(zip(g0[i, :k].tolist(), g1[i, :k].tolist()))) == k
                if f["spread"] == "first_slab":                  # all of it in the first slab, at even distances: a buffer to each key
                    first = np.array([np.flatnonzero((g0[i] == a) & (g1[i] == b))[0] for a, b in zip(*cc.keys_at(T, f["home"], f["chain"]))])
                    assert M.slab_counts[i, 0] == f["chain"] and (np.diff(first) >= 260 // f["chain"]).all()     # while the slab has that many
                    if f["chain"] <= cc.slab_buffers(G, 0):
                        assert len(set((first // G.buffer).tolist())) == f["chain"]
                if f["spread"] == "slabs":
                    assert (M.slab_counts[i, [g for g, s in enumerate(G.slab_sizes) if s]] >= 1).all() and M.slab_counts[i].max() < f["chain"]
            if M.names[i] == "plain":
                assert M.counts[i] <= cc.PLAIN_CLASSES and M.expect[i] == "coded"
                assert len(set(home[i].tolist())) == M.counts[i]               # home slots of their own: a plain SNP never probes twice
            elif f.get("own_homes"):                              # exactly drows classes and no probing: nothing excuses giving it up
                assert f["count"] == G.drows == len(set(home[i].tolist())) and M.expect[i] == "coded"
            elif "count" in f and "group" not in f:
                assert M.expect[i] == cc.expectation_of_count(G, f["count"])
        # every adversarial SNP has plain neighbours in its wavefront (SNP 63 of a tile and SNP 0 of the next never share one)
        adv = M.names != "plain"
        if M.name != "groups":
            assert not (adv[1:] & adv[:-1] & (np.arange(1, M.m) % 64 != 0)).any()
            assert all((~adv[i - i % 4:i - i % 4 + 4]).any() for i in np.flatnonzero(adv))
            # every case at every required position of a tile, and in the last, partial tile
            for name in sorted(set(M.names[adv]) - {"ballast"}):
                at = np.flatnonzero(M.names == name)
                assert set(cc.POSITIONS) <= set((at[M.where[at] == "tile"] % 64).tolist()), (M.name, name)
                assert (at[M.where[at] == "partial"] >= 64 * (M.m // 64)).sum() >= 1, (M.name, name)
                seen_cases.add(name)
            # the scoring group rule never has a say here: no aligned group of SNPs that may stay coded exceeds its cap
            eff = np.where(M.expect == "rich", 0, M.counts)
            eff = np.concatenate([eff, np.zeros(-M.m % 64, dtype=eff.dtype)])
            for batch in (4, 8, 16):
                assert eff.reshape(-1, batch).sum(axis=1).max() <= cc.BATCH_ROWS_CAP
        else:
            batch = G.score_batch
            for kind, total in (("exact", cc.BATCH_ROWS_CAP), ("over", cc.BATCH_ROWS_CAP + 1), ("tie", cc.BATCH_ROWS_CAP + 1)):
                at = np.flatnonzero(M.names == "group_" + kind)
                starts = at[::batch]
                assert len(at) == 3 * batch and (starts % batch == 0).all() and np.array_equal(at.reshape(3, batch), starts[:, None] + np.arange(batch))
                assert {0, 64 - batch} <= set((starts % 64).tolist()) and (starts >= 64 * (M.m // 64)).sum() == 1
                for s in starts:
                    c, e = M.counts[s:s + batch], M.expect[s:s + batch]
                    assert c.sum() == total and c.max() <= G.limit()
                    assert len(set(home[s + int(np.argmax(c))].tolist())) == c.max()        # no probing: only the rule can make it rich
                    if kind == "exact":
                        assert (e == "coded").all()
                    else:
                        assert (e == "rich").sum() == 1 and e[int(np.argmax(c))] == "rich"  # the richest, the lowest lane on ties
                        assert (c == c.max()).sum() == (3 if kind == "tie" else 1)
        # the sample pass (every SNP through a 256-slot table; a SNP it gives up counts as 255): fewer than 1 % of the SNPs at 200 or
        # more even if every long chain is given up, so the matrix is coded; more than 0.1 % at 250 or more, so drows = T - T/8
        worst = np.sort(np.where([cc.heavy(type("R", (), {"facts": f})) for f in M.facts], 255, M.counts))
        assert worst[int(np.ceil(0.99 * M.m)) - 1] < 200
        if M.name == "groups":
            g99 = np.sort(M.counts)[int(np.ceil(0.99 * M.m)) - 1]
            assert {16: g99 * 16 <= 616, 8: g99 * 8 <= 616, 4: True}[G.score_batch]
            g999 = np.sort(M.counts)[int(np.ceil(0.999 * M.m)) - 1]
            assert min(254, T - T // 8, (g999 + 11) & ~7) >= M.counts.max()
        else:
            assert np.sort(M.counts)[int(np.ceil(0.999 * M.m)) - 1] >= 250
    want = {"chain_%d_%s_%s" % (c, h, s) for c in cc.CHAIN_LENGTHS for h in cc.CHAIN_HOMES for s in cc.CHAIN_SPREADS}
    want |= {"count_%d" % c for c in (T, T + 1, T - T // 8, T - T // 8 + 1, 8, 9, 16, 17, 24, 25, 63, 64, 65, 127, 128, 129, 253, 254, 255, 256)}
    want |= {"count_%d_spread" % G.drows}
    want |= {"lanes_new_key_fills_a_quad", "lanes_new_key_fills_a_buffer", "lanes_two_new_keys_one_home", "appear_in_a_quad_straddling_a_slab_end",
             "appear_after_an_empty_slab", "appear_slab_of_high_classes_only", "appear_last_of_slab_of_5_and_matrix", "bits_lowest_mantissa_bit_of_g0",
             "bits_lowest_mantissa_bit_of_g1", "bits_swapped_pair", "bits_signed_zeros", "bits_nan_payloads", "bits_key_empty"}
    want |= {"appear_last_of_slab_of_%d" % s for s in (1, 3, 4, G.buffer - 1, G.buffer + 1)}
    assert want <= seen_cases, sorted(want - seen_cases)


@pytest.mark.parametrize("T", cc.GEOMETRIES)
def test_the_order_matrix_keeps_its_claims(T):
    """Every slab is one quad -- all of a SNP's individuals fall in column 0's walk, whatever the geometry --, the stated ranks are
    first-appearance ranks, every kind of row stands at every required lane position, and the sample pass will code the matrix."""
    M = cc.order_matrix(T)
    G = M.G
    assert M.L.shape == (cc.ORDER_M, 2 * G.n) and M.m % 64 != 0 and max(G.slab_sizes) <= 4 and 0 in G.slab_sizes
    assert sum(1 for s in G.slab_sizes if s == 4) >= 2 and {1, 2, 3} <= set(G.slab_sizes)
    Lb = M.L.view(np.uint32)
    g0, g1 = Lb[:, 0::2], Lb[:, 1::2]
    home = cc.home_slot(g0, g1, T)
    for i in range(M.m):
        pairs = list(zip(g0[i].tolist(), g1[i].tolist()))
        order = sorted(set(pairs), key=pairs.index)
        assert M.rank[i].tolist() == [order.index(p) for p in pairs] and M.counts[i] == len(order) == M.rank[i].max() + 1
        if "chain" in M.facts[i]:
            assert M.counts[i] == G.n and (home[i] == M.facts[i]["home"]).all()
    assert M.counts[M.names == "order_all_new"].min() == G.n and M.counts[M.names == "order_one_class"].max() == 1
    assert (M.rank[M.names == "order_new_in_the_last"] == np.arange(G.n) // (G.n - 1)).all()
    assert (M.counts[M.names == "order_random"] >= 2).all() and len(set(M.counts[M.names == "order_random"].tolist())) >= 6
    for name in sorted(set(M.names)):
        at = np.flatnonzero(M.names == name)
        assert set((at[at < 64 * (M.m // 64)] % 64).tolist()) == set(range(64)), name      # (so at each of cc.POSITIONS)
        assert (at >= 64 * (M.m // 64)).any(), name
    assert M.counts.max() <= 24 and M.counts.max() * 16 <= cc.BATCH_ROWS_CAP and (M.expect == "coded").all()


@pytest.mark.parametrize("T", cc.GEOMETRIES)
def test_the_sparse_chain_matrix_keeps_its_claims(T):
    """Chains that must be coded -- ENC_RMAX keys, and 16 that wrap past the last slot -- in so few SNPs that the sample pass codes
    the matrix even if it gave every one of them up."""
    M = cc.sparse_chain_matrix(T)
    G = M.G
    Lb = M.L.view(np.uint32)
    home = cc.home_slot(Lb[:, 0::2], Lb[:, 1::2], T)
    at = np.flatnonzero(M.names != "plain")
    assert at.tolist() == sorted(cc.SPARSE_SEATS) and M.m == cc.SPARSE_M and M.m % 64 != 0 and (M.expect == "coded").all()
    assert {0, 63} <= set((at % 64).tolist()) and (at >= 64 * (M.m // 64)).sum() == 2
    chains, homes = set(), set()
    for i in at:
        f = M.facts[i]
        assert M.counts[i] == f["chain"] <= cc.ENC_RMAX and (home[i] == f["home"]).all()
        chains.add(f["chain"])
        homes.add(f["home"])
    assert chains == {16, cc.ENC_RMAX} and homes == {5, T - 1, T - 2}
    worst = np.sort(np.where(M.names != "plain", 255, M.counts))
    assert worst[int(np.ceil(0.99 * M.m)) - 1] < 200 and M.counts.max() == cc.ENC_RMAX


@pytest.mark.parametrize("T", cc.GEOMETRIES)
def test_digests(T):
    assert cc.order_matrix(T).digest() == ORDER_DIGESTS[T]
    assert cc.sparse_chain_matrix(T).digest() == SPARSE_DIGESTS[T]
    got = {(T, M.name): M.digest() for M in cc.build(T)}
    assert got == {k: v for k, v in DIGESTS.items() if k[0] == T}, got
