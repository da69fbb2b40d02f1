"""The serial restatement of the `--scaffold` rules (tests/scaffold_cases.py::expected_scaffolds) held against properties that do
not use its walk: every unitig placed once, neighbours joined by a link that a separate loop finds strong and unique at both
ends, every gap the formula's, no dependence on the order of the links, and the strand of a unitig following the names of its
ends.  No GPU here; tests/test_gpu_scaffold.py holds the device against the same restatement."""
import random

import pytest

from tests import chimeric_cases as cc
from tests import pair_cases as pp
from tests import scaffold_cases as sc

B, E = sc.B, sc.E


def _all_inputs():
    for name, res, links, opts in sc.hand_built():
        yield name, res, links, [0] * 24, opts
    for seed in range(200):
        res, links, st24, opts = sc.random_links_case(seed)
        yield "random%d" % seed, res, links, st24, opts
    res, links, _, _ = sc.shuffled_chain(300, 5)
    yield "chain300", res, links, [0] * 24, {"insert_size": 100}


def _unique_strong(links, nu, res, o):
    """the joins, recomputed without expected_scaffolds' tables: a quadratic loop over the links -> {frozenset(a, b): link}"""
    cand = [ln for ln in links if sc.link_class(ln, nu, res["seq_offs"], res["uflags"], o) == "CANDIDATE"]

    def strong(ln):
        if o["link_ratio"] == 0:
            return True
        for e in ln[:2]:
            if any(e in other[:2] and ln[2] * o["link_ratio"] <= other[2] for other in cand):
                return False
        return True

    strongs = [ln for ln in cand if strong(ln)]
    out = {}
    for ln in strongs:
        if all(sum(1 for other in strongs if e in other[:2]) == 1 for e in ln[:2]):
            out[frozenset(ln[:2])] = ln
    return out


def _check(name, res, links, st24, opts):
    o = dict(sc.DEFAULT_OPTS, **opts)
    exp = sc.expected_scaffolds(res, links, st24, opts)
    nu = len(res["uflags"])
    ins = sc.insert_from_status(st24) if o["insert_size"] is None else o["insert_size"]
    bases = [res["seq_offs"][u + 1] - res["seq_offs"][u] for u in range(nu)]
    # every unitig in exactly one scaffold, exactly once
    assert sorted(p[0] for p in exp["layout"]) == list(range(nu)), name
    assert exp["sc_lay_offs"][0] == 0 and exp["sc_lay_offs"][-1] == nu and len(exp["sc_flags"]) == exp["status"][0]
    joins = _unique_strong(sc._plain(links), nu, res, o)
    used = 0
    firsts = []
    for s in range(exp["status"][0]):
        lay = exp["layout"][exp["sc_lay_offs"][s]:exp["sc_lay_offs"][s + 1]]
        assert lay and lay[0][2] == 0, name
        firsts.append(lay[0][0])
        ends = lambda p: (2 * p[0] + (E if p[1] else B), 2 * p[0] + (B if p[1] else E))  # noqa: E731  (entered through, left through)
        for x, y in zip(lay, lay[1:]):
            key = frozenset((ends(x)[1], ends(y)[0]))
            assert key in joins, (name, s, x, y)
            gap, _, _ = sc.gap_of(joins[key], ins, o)
            assert o["min_gap"] <= gap <= o["max_gap"]
            assert y[2] == x[2] + bases[x[0]] + gap, (name, s)
            used += 1
        assert exp["sc_offs"][s + 1] - exp["sc_offs"][s] == lay[-1][2] + bases[lay[-1][0]], name
        if exp["sc_flags"][s] & 1:  # a ring: the closing join leads from the last unitig back to the first, which is the smallest
            key = frozenset((ends(lay[-1])[1], ends(lay[0])[0]))
            assert key in joins and sc.gap_of(joins[key], ins, o)[0] == exp["sc_flags"][s] >> 1, name
            assert lay[0][0] == min(p[0] for p in lay) and lay[0][1] == 0
            used += 1
        else:  # a path: its ends are free, it starts at the smaller terminal, and a single unitig lies forward
            assert exp["sc_flags"][s] == 0
            assert not any(ends(lay[0])[0] in k for k in joins) and not any(ends(lay[-1])[1] in k for k in joins), name
            assert lay[0][0] <= lay[-1][0] and (len(lay) > 1 or lay[0][1] == 0)
        if any(res["uflags"][p[0]] & 1 for p in lay):
            assert len(lay) == 1 and exp["sc_flags"][s] == 0
    assert used == len(joins) and firsts == sorted(firsts), name
    assert exp["status"][10] + exp["status"][11] == len(joins)
    # the bases: the unitigs as placed, N in the gaps
    seqs, useqs = exp["seqs"], res["useqs"]
    assert len(seqs) == exp["sc_offs"][-1] == exp["status"][1]
    covered = 0
    for s in range(exp["status"][0]):
        for p in exp["layout"][exp["sc_lay_offs"][s]:exp["sc_lay_offs"][s + 1]]:
            at = exp["sc_offs"][s] + p[2]
            src = useqs[res["seq_offs"][p[0]]:res["seq_offs"][p[0] + 1]]
            assert seqs[at:at + len(src)] == (sc.uc.revcomp(src) if p[1] else src), name
            covered += len(src)
    assert exp["status"][12] == len(seqs) - covered
    return exp


def test_properties_of_the_restatement():
    seen = [0] * 16
    for name, res, links, st24, opts in _all_inputs():
        exp = _check(name, res, links, st24, opts)
        seen = [a + b for a, b in zip(seen, exp["status"])]
    assert all(seen[k] > 0 for k in range(15)), seen


def test_link_order_does_not_matter():
    for name, res, links, st24, opts in _all_inputs():
        exp = sc.expected_scaffolds(res, links, st24, opts)
        rng = random.Random(len(links))
        for other in (links[::-1], rng.sample(links, len(links))):
            got = sc.expected_scaffolds(res, other, st24, opts)
            assert all(got[k] == exp[k] for k in ("sc_offs", "sc_lay_offs", "sc_flags", "layout", "seqs", "status")), name


def test_renaming_the_ends_of_a_unitig_flips_it():
    """e -> e ^ 1 on one unitig, its bases reverse-complemented with it: that unitig's placement flips, the scaffolds' bases stay
    -- unless the unitig starts a scaffold, which then runs the other way or, for a unitig on its own, stays as it is"""
    for name, res, links, st24, opts in _all_inputs():
        nu = len(res["uflags"])
        exp = sc.expected_scaffolds(res, links, st24, opts)
        lay_of = {p[0]: p for p in exp["layout"]}
        for u in range(min(nu, 6)):
            so = res["seq_offs"]
            swapped = dict(res, useqs=res["useqs"][:so[u]] + sc.uc.revcomp(res["useqs"][so[u]:so[u + 1]]) + res["useqs"][so[u + 1]:])
            ren = lambda e: e ^ 1 if e >> 1 == u and e < 2 * nu else e  # noqa: E731
            other = []
            for a, b, c, mn, sm in sc._plain(links):
                ok = a < b  # (a record that is malformed by its order stays so)
                a, b = ren(a), ren(b)
                other.append((min(a, b), max(a, b), c, mn, sm) if ok else (max(a, b), min(a, b), c, mn, sm))
            got = sc.expected_scaffolds(swapped, other, st24, opts)
            s = next(k for k in range(exp["status"][0]) if exp["sc_lay_offs"][k] <= exp["layout"].index(lay_of[u]) < exp["sc_lay_offs"][k + 1])
            lay = exp["layout"][exp["sc_lay_offs"][s]:exp["sc_lay_offs"][s + 1]]
            if len(lay) == 1 or exp["sc_flags"][s] & 1 and lay[0][0] == u:
                continue  # a single unitig is forward under either naming; a ring's start is forward and the ring turns round
            assert got["status"] == exp["status"] and got["sc_offs"] == exp["sc_offs"], (name, u)
            assert got["layout"] == [(p[0], p[1] ^ (p[0] == u), p[2]) for p in exp["layout"]], (name, u)
            assert got["seqs"] == exp["seqs"], (name, u)


@pytest.mark.parametrize("name", [c[0] for c in sc.hand_built()])
def test_hand_built(name):
    _, res, links, opts = sc.case_named(name)
    exp = _check(name, res, links, [0] * 24, opts)
    st = exp["status"]
    if name.startswith("sizes"):
        assert st[0] == 1 and st[10] == 6 and exp["gaps"] == [0, 1, 15, 16, 17, 3, 2] and st[12] == 54
    if name == "gap_in_a_piece":
        assert exp["gaps"] == [0, 3, 1] and [p[2] for p in exp["layout"]] == [0, 23, 44]
    if name == "cycle3":
        assert st[0] == 1 and st[11] == 1 and st[10] == 2 and exp["sc_flags"] == [1 | (30 << 1)] and [p[0] for p in exp["layout"]][0] == 0
    if name == "cycle70":
        assert st[11] == 1 and st[10] == 69 and st[0] == 1
    if name == "cycle_and_path":
        assert st[0] == 2 and st[11] == 1 and exp["sc_lay_offs"] == [0, 3, 7]
        assert exp["layout"][0][0] == 1 and exp["layout"][3][0] == 5  # the ring starts at 1; the path 6 0 3 5 at 5, the smaller terminal
    if name == "circular_unitig":
        assert st[5] == 2 and st[10] == 1 and st[0] == 2  # 1-2 and 3-4 touch the circular unitig; 1-4 joins unitigs 0 and 2 past it
    if name == "turned":
        assert [p[0] for p in exp["layout"]] == [1, 2, 0, 3]


def test_precedence_thresholds_and_gaps():
    res = sc.make_res([30, 40, 50, 60], circular=(3,), seed=3)
    o = {"insert_size": 100, "min_pairs": 2, "min_unitig_bases": 31}
    # one link per class in precedence order; a link that is SELF and THIN counts as SELF, CIRCULAR before SHORT before THIN
    links = [(9, 2, 5, 1, 5), (2, 3, 1, 1, 1), (0, 6, 1, 1, 1), (1, 2, 1, 1, 1), (3, 4, 1, 50, 50), (3, 5, 2, 50, 100)]
    st = sc.expected_scaffolds(res, links, [0] * 24, o)["status"]
    assert st[3:8] == [1, 1, 1, 1, 1] and st[10] == 1
    for mb, joined in ((40, 1), (41, 0)):  # min_unitig_bases at exactly bases(u) and one above
        st = sc.expected_scaffolds(res, [sc.link(3, 4)], [0] * 24, dict(o, min_unitig_bases=mb))["status"]
        assert st[10] == joined and st[6] == 1 - joined
    assert sc.expected_scaffolds(res, [sc.link(3, 4, count=1)], [0] * 24, dict(o, min_pairs=1))["status"][10] == 1
    twice = sc.expected_scaffolds(res, [sc.link(3, 4)] * 2, [0] * 24, o)["status"]
    assert twice[9] == 2 and twice[10] == 0
    # m == insert_size, m == insert_size - 1, the clamp, a sum near 2^63, insert_size from the status with a remainder
    for span, ins, gap, below, clamped in ((100, 100, 1, 1, 0), (99, 100, 1, 0, 0), (10, 100, 60, 0, 1), ((1 << 62) - 100, (1 << 62) - 93, 7, 0, 0)):
        e = sc.expected_scaffolds(res, [(3, 4, 2, 9, 2 * span + 1)], [0] * 24, dict(o, insert_size=ins, max_gap=60))
        assert (max(e["gaps"]) if e["status"][10] else None, e["status"][13], e["status"][14]) == (gap, below, clamped)
    st24 = [0] * 24
    st24[14], st24[15] = 3, 500  # 166 and a remainder
    e = sc.expected_scaffolds(res, [sc.link(3, 4, span=100)], st24, dict(o, insert_size=None))
    assert 66 in e["gaps"]
    st24[14] = 0
    e = sc.expected_scaffolds(res, [sc.link(3, 4, span=100)], st24, dict(o, insert_size=None))
    assert e["status"][13] == 1 and 1 in e["gaps"]


def test_contended_ends():
    res = sc.make_res([20] * 301, seed=4)
    many = [sc.link(1, 2 * u, count=4) for u in range(1, 301)]
    o = {"insert_size": 200}
    for ratio, weak, ambiguous in ((0, 0, 300), (1, 300, 0), (2, 0, 300)):  # ties: with ratio 1 a link is weak against itself
        st = sc.expected_scaffolds(res, many, [0] * 24, dict(o, link_ratio=ratio))["status"]
        assert (st[8], st[9], st[10]) == (weak, ambiguous, 0)
    one = [sc.link(1, 2, count=9)] + many[1:]
    st = sc.expected_scaffolds(res, one, [0] * 24, dict(o, link_ratio=2))["status"]
    assert (st[8], st[9], st[10], st[0]) == (299, 0, 1, 300)


def test_random_graphs_through_the_calls_reach_every_count():
    """the inputs of the GPU test's hundred graphs, serially: status entries 4, 7, 8, 9, 10 and 13 each occur"""
    seen = [0] * 16
    for seed in range(100):
        case = pp.random_case(seed)
        res = cc.run(cc.expected_chimeric, case)
        pairs = pp.expected_pairs(res, [len(r) for r in case["reads"]], case["mate"], {"max_span": 0})
        links = pairs["links"] + sc.pipeline_extra_links(seed, len(res["uflags"]), pairs["links"])
        exp = _check(case["name"], dict(res, useqs=bytes(res["useqs"])), links, pairs["status"], sc.pipeline_options(seed))
        seen = [a + b for a, b in zip(seen, exp["status"])]
    assert all(seen[k] > 0 for k in (4, 7, 8, 9, 10, 13)), seen
