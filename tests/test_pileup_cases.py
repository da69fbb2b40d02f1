"""The serial restatement of `siga correct -a overlap` (tests/pileup_cases.py) pinned by hand-computed answers, rule by rule,
and its seeded candidate search against the search without seeds.  No GPU."""
from tests import pileup_cases as pc

G = pc.random_genome(400, 77)


def test_seed_positions():
    assert pc.seed_positions(23, 24, 12) == []
    assert pc.seed_positions(24, 24, 12) == [0]
    assert pc.seed_positions(25, 24, 12) == [0, 1]
    assert pc.seed_positions(48, 24, 12) == [0, 12, 24]
    assert pc.seed_positions(50, 24, 12) == [0, 12, 24, 26]
    assert pc.seed_positions(30, 12, 1) == list(range(19))


def test_seeded_and_brute_force_candidates_agree():
    case = pc.seedable_case()
    p = case["params"]
    seen, strands = 0, set()
    for q in case["queries"]:
        cands, _, _, _ = pc.seed_candidates(case["refs"], q, p)
        got = {c for c in cands if pc.accepted(case["refs"], q, c, p)}
        want = pc.brute_candidates(case["refs"], q, p)
        assert got == want
        seen += len(want)
        strands |= {c[1] for c in want}
    assert seen > 20 and strands == {0, 1}


def test_diagonals_and_strands_by_hand():
    core = G[100:160]  # the query
    refs = [G[90:150],            # starts 10 before the query: d = +10
            G[100:160],           # the query itself: d = 0
            G[110:170],           # starts 10 into the query: d = -10
            G[105:155],           # inside the query: d = -5
            G[80:180],            # around the query: d = +20
            pc.revcomp(G[90:150]),   # the first one on the other strand: d = +10 against its reverse complement
            pc.revcomp(G[105:155]),
            pc.revcomp(G[80:180])]
    p = pc.params(S=12, T=6, M=40, P=0, C=3, D=1)
    cands, located, repeats, listed = pc.seed_candidates(refs, core, p)
    assert cands == {(0, 0, 10), (1, 0, 0), (2, 0, -10), (3, 0, -5), (4, 0, 20), (5, 1, 10), (6, 1, -5), (7, 1, 20)}
    assert located == len(pc.seed_positions(60, 12, 6)) == 9 and repeats == 0
    assert all(pc.accepted(refs, core, c, p) for c in cands)
    q2, valid, st = pc.pile_one(refs, core, p)
    assert (q2, valid) == (core, 1) and st[5] == st[6] == 8 and st[7] == 0 and st[0] == listed
    # column 0 is covered by reads 0, 1, 4, 5, 7; column 59 by 1, 2, 4, 7
    x0, x1, _, m = pc.overlap_of(refs, core, (2, 0, -10))
    assert (x0, x1, m) == (10, 60, 0)
    x0, x1, _, m = pc.overlap_of(refs, core, (0, 0, 10))
    assert (x0, x1, m) == (0, 50, 0)


def test_acceptance_edges():
    q = G[100:160]
    refs = [G[115:200]]  # overlap: columns 15 .. 59, l = 45
    assert pc.accepted(refs, q, (0, 0, -15), pc.params(M=45, P=0))
    assert not pc.accepted(refs, q, (0, 0, -15), pc.params(M=46, P=0))
    bad = pc.mutate(q, [20, 30])  # two mismatches in the overlap: floor(45 * P / 1000) = 2 from P = 45 (2025 / 1000), 1 at P = 44
    assert pc.accepted(refs, bad, (0, 0, -15), pc.params(M=45, P=45))
    assert not pc.accepted(refs, bad, (0, 0, -15), pc.params(M=45, P=44))
    assert not pc.accepted(refs, bad, (0, 0, -15), pc.params(M=45, P=0))
    withn = q[:20] + "N" + q[21:]  # a byte outside ACGT is a mismatch
    assert pc.overlap_of(refs, withn, (0, 0, -15))[3] == 1


def test_one_triple_through_many_seeds_and_a_tandem_repeat():
    q = G[100:160]
    p = pc.params(S=12, T=1, M=20, P=0, C=1, D=1)
    cands, located, _, listed = pc.seed_candidates([q], q, p)
    assert cands == {(0, 0, 0)} and located == listed == 49
    unit = G[0:30]
    rep = unit + unit + G[200:220]  # the unit twice: a read of the unit's bases lies on it at two diagonals
    cands, _, _, _ = pc.seed_candidates([rep], unit, p)
    assert cands == {(0, 0, 0), (0, 0, 30)}
    q2, valid, st = pc.pile_one([rep], unit, p)
    assert st[5] == st[6] == 2 and valid == 1 and q2 == unit


def _vote_case(n_good, n_bad):
    """a query with a substitution at column 30; n_good reads say the genome's base, n_bad reads carry the query's"""
    q = pc.mutate(G[100:160], [30])
    refs = [G[100 - i:160 + i] for i in range(1, n_good + 1)] + [pc.mutate(G, [130])[100 - i:160 + i] for i in range(20, 20 + n_bad)]
    return q, refs


def test_vote_edges():
    p = pc.params(S=12, T=6, M=40, P=50, C=3, D=1)
    want = G[100:160]
    q, refs = _vote_case(3, 2)  # cnt[c] = C, cnt[b] = C - 1: changed
    assert pc.pile_one(refs, q, p)[:2] == (want, 1)
    q, refs = _vote_case(2, 1)  # cnt[c] = C - 1: not changed
    assert pc.pile_one(refs, q, p)[:2] == (q, 1)
    q, refs = _vote_case(4, 3)  # cnt[b] = C: not changed
    assert pc.pile_one(refs, q, p)[:2] == (q, 1)
    q, refs = _vote_case(3, 3)  # a tie for the largest count
    assert pc.pile_one(refs, q, pc.params(S=12, T=6, M=40, P=50, C=3, D=1))[:2] == (q, 1)
    q, refs = _vote_case(3, 3)
    assert pc.pile_one(refs, q, pc.params(S=12, T=6, M=40, P=50, C=4, D=1))[:2] == (q, 1)


def test_depth_and_n():
    q = G[100:160]
    refs = [G[100:160], G[100:160], G[110:200]]  # columns 0..9: two reads, columns 10..59: three
    p = pc.params(S=12, T=6, M=40, P=50, C=2, D=2)
    assert pc.pile_one(refs, q, p)[:2] == (q, 1)
    assert pc.pile_one(refs, q, pc.params(S=12, T=6, M=40, P=50, C=2, D=3))[:2] == (q, 0)
    withn = q[:30] + "N" + q[31:]  # an N in the query: replaced; the seeds that hold it are skipped
    q2, valid, st = pc.pile_one(refs, withn, p)
    assert (q2, valid) == (q, 1) and st[7] == 1
    assert st[3] == sum(1 for s in pc.seed_positions(60, 12, 6) if not s <= 30 < s + 12)
    alln = "N" * 60  # every seed skipped: no pile, not valid
    assert pc.pile_one(refs, alln, p) == (alln, 0, [0] * 8)


def test_caps_and_lengths():
    q = G[100:160]
    refs = [q] * 5
    p = pc.params(S=12, T=6, M=40, P=0, C=2, D=1)
    assert pc.pile_one(refs, q, pc.params(S=12, T=6, M=40, P=0, C=2, D=1, H=5))[1] == 1   # a seed at H hits
    got = pc.pile_one(refs, q, pc.params(S=12, T=6, M=40, P=0, C=2, D=1, H=4))            # at H + 1: every seed a repeat
    assert got[1] == 0 and got[2][3] == got[2][4] == 9 and got[2][0] == 0
    assert pc.pile_one(refs, q, pc.params(S=12, T=6, M=40, P=0, C=2, D=1, K=5))[1] == 1   # K distinct candidates
    got = pc.pile_one(refs, q, pc.params(S=12, T=6, M=40, P=0, C=2, D=1, K=4))            # K + 1
    assert got[:2] == (q, 0) and got[2][2] == 1 and got[2][5] == 0
    assert pc.pile_one(refs, q[:11], p) == (q[:11], 0, [0] * 8)                           # S - 1
    assert pc.pile_one(refs, q[:12], pc.params(S=12, T=6, M=12, P=0, C=2, D=1))[1] == 1   # S
    got = pc.pile_one(refs, q, pc.params(S=12, T=6, M=40, P=0, C=2, D=1, max_len=59))
    assert got[:2] == (q, 2) and got[2][1] == 1


def test_rounds():
    """three substitutions inside the first 20 bases of a 100-base read at 20-fold cover: one round repairs all three (the
    seeds further along find the pile and every column is voted from the same pile); and a case where round 2 changes a base
    round 1 could not: with P tight, a read over the whole query is accepted only once round 1 has repaired two of the mismatches it saw"""
    g = pc.random_genome(600, 9)
    truth = g[200:300]
    q = pc.mutate(truth, [3, 9, 17])
    refs = [g[200 - 5 * i:300 - 5 * i] for i in range(-10, 11) if i]  # 20 reads, a start every 5 bases around the query
    p = pc.params(S=24, T=12, M=45, P=40, C=5, D=2)
    one = pc.expected_pileup(refs, [q], p, rounds=1)
    assert one["seqs"] == [truth] and one["valid"] == [1] and one["changed"] == [1] and one["status"][7] == 3
    more = pc.expected_pileup(refs, [q], p, rounds=5)
    assert more["seqs"] == [truth] and more["rounds_run"] == 2 and more["per_round"][1][7] == 0
    case = pc.second_round_case()
    r1 = pc.expected_pileup(case["refs"], case["queries"], case["params"], rounds=1)
    r2 = pc.expected_pileup(case["refs"], case["queries"], case["params"], rounds=3)
    assert r1["seqs"] != r2["seqs"] and r2["per_round"][1][7] >= 1 and r2["seqs"] == [case["truth"]]
