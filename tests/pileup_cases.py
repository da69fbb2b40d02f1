"""`siga correct -a overlap`: the rules of include/sigax.h (the pile-up block) restated serially, with Python integers and
strings, and the cases of tests/test_pileup_cases.py and tests/test_gpu_overlap_correct.py.  No tests here.

expected_pileup()   rules 1-8: seeds, candidates, acceptance, votes, change, validity, rounds -> sequences, valid, changed and
                    the eight status words of every round
seed_candidates()   rules 2-3 alone: the distinct (read, strand, diagonal) triples the seeds of a query find
brute_candidates()  the acceptable triples found by trying every read, strand and diagonal, without seeds
case builders       random genomes with reads of mixed lengths on both strands, and the two-round case
"""
import random

PILE_MAX_LEN = 4096
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}

# the defaults of the CLI
DEFAULTS = dict(S=24, T=12, H=256, M=45, P=40, C=5, D=2, K=512, max_len=PILE_MAX_LEN)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def acgt(s):
    return all(c in "ACGT" for c in s)


def seed_positions(n, S, T):
    """rule 2: p = 0, T, 2T, ... while p + S <= n, then n - S if it is not among them"""
    if n < S:
        return []
    ps = list(range(0, n - S + 1, T))
    if ps[-1] != n - S:
        ps.append(n - S)
    return ps


def occurrences(refs, w):
    """[(t, o)] with refs[t][o:o+len(w)] == w"""
    out = []
    for t, r in enumerate(refs):
        o = r.find(w)
        while o >= 0:
            out.append((t, o))
            o = r.find(w, o + 1)
    return out


def seed_candidates(refs, q, p):
    """rules 2-3 -> (set of (t, strand, d), seeds located, seeds skipped as repeats, hits listed)"""
    S, T, H = p["S"], p["T"], p["H"]
    cands = set()
    located = repeats = listed = 0
    for pos in seed_positions(len(q), S, T):
        w = q[pos:pos + S]
        if not acgt(w):
            continue
        located += 1
        fwd = occurrences(refs, w)
        rev = occurrences(refs, revcomp(w))
        if len(fwd) + len(rev) > H:
            repeats += 1
            continue
        listed += len(fwd) + len(rev)
        for t, o in fwd:
            cands.add((t, 0, o - pos))
        for t, o in rev:
            cands.add((t, 1, len(refs[t]) - o - S - pos))
    return cands, located, repeats, listed


def overlap_of(refs, q, cand):
    """rule 4 -> (x0, x1, text of the candidate as the query faces it, mismatches)"""
    t, strand, d = cand
    text = revcomp(refs[t]) if strand else refs[t]
    x0, x1 = max(0, -d), min(len(q), len(text) - d)
    m = sum(1 for x in range(x0, x1) if q[x] != text[x + d])
    return x0, x1, text, m


def accepted(refs, q, cand, p):
    x0, x1, _, m = overlap_of(refs, q, cand)
    ell = x1 - x0
    return ell >= p["M"] and m <= (ell * p["P"]) // 1000


def brute_candidates(refs, q, p):
    """every (t, strand, d) with an overlap that rule 4 accepts, found without seeds"""
    out = set()
    for t, r in enumerate(refs):
        for strand in (0, 1):
            for d in range(-len(q) + 1, len(r)):
                c = (t, strand, d)
                x0, x1, _, _ = overlap_of(refs, q, c)
                if x1 - x0 >= 1 and accepted(refs, q, c, p):
                    out.add(c)
    return out


def pile_one(refs, q, p):
    """rules 1-7 for one query -> (q', valid, status8 as a list; status[0] = the hits its seeds list)"""
    st = [0] * 8
    n = len(q)
    if n < p["S"]:
        return q, 0, st
    if n > min(p["max_len"], PILE_MAX_LEN):
        st[1] = 1
        return q, 2, st
    cands, located, repeats, listed = seed_candidates(refs, q, p)
    st[0], st[3], st[4] = listed, located, repeats
    if len(cands) > p["K"]:
        st[2] = 1
        return q, 0, st
    cnt = [dict.fromkeys("ACGT", 0) for _ in range(n)]
    for c in sorted(cands):
        st[5] += 1
        if not accepted(refs, q, c, p):
            continue
        st[6] += 1
        x0, x1, text, _ = overlap_of(refs, q, c)
        for x in range(x0, x1):
            cnt[x][text[x + c[2]]] += 1
    out = []
    for x in range(n):
        b = q[x]
        cb = cnt[x].get(b, 0)
        top = max(cnt[x].values())
        best = [c for c in "ACGT" if cnt[x][c] == top]
        nb = b
        if len(best) == 1 and best[0] != b and top >= p["C"] and cb < p["C"]:
            nb = best[0]
        out.append(nb)
    valid = 1 if all(cnt[x].get(out[x], 0) >= p["D"] for x in range(n)) else 0
    if not valid:
        return q, 0, st
    qn = "".join(out)
    st[7] = sum(1 for a, b in zip(q, qn) if a != b)
    return qn, 1, st


def expected_round(refs, queries, p):
    """one round over every query -> (sequences, valid, changed, status8)"""
    outs, valid, changed, st = [], [], [], [0] * 8
    for q in queries:
        qn, v, s = pile_one(refs, q, p)
        outs.append(qn)
        valid.append(v)
        changed.append(1 if qn != q else 0)
        st = [a + b for a, b in zip(st, s)]
    return outs, valid, changed, st


def expected_pileup(refs, queries, p, rounds=1):
    """rules 1-8 -> dict: seqs, valid, changed (in any round), status (the rounds' words added up), rounds_run, per_round"""
    seqs = list(queries)
    valid = [0] * len(seqs)
    changed = [0] * len(seqs)
    total = [0] * 8
    active = list(range(len(seqs)))
    per_round = []
    run = 0
    while run < rounds and active:
        outs, v, ch, st = expected_round(refs, [seqs[i] for i in active], p)
        run += 1
        per_round.append(st)
        total = [a + b for a, b in zip(total, st)]
        nxt = []
        for k, i in enumerate(active):
            seqs[i], valid[i] = outs[k], v[k]
            if ch[k]:
                changed[i] = 1
                nxt.append(i)
        active = nxt
    return dict(seqs=seqs, valid=valid, changed=changed, status=total, rounds_run=run, per_round=per_round)


# ---- case builders --------------------------------------------------------------------------------------------------------------
def random_genome(n, seed):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(s, positions):
    """substitute s at the positions with the next base of ACGT"""
    t = list(s)
    for x in positions:
        t[x] = "ACGT"[("ACGT".index(t[x]) + 1) % 4]
    return "".join(t)


def sample_reads(genome, n_reads, lens, seed, rc=True):
    """reads of the lengths of `lens` (cycled) from random places of the genome, every other one reverse-complemented"""
    rng = random.Random(seed)
    out = []
    for i in range(n_reads):
        L = lens[i % len(lens)]
        o = rng.randrange(0, len(genome) - L + 1)
        r = genome[o:o + L]
        out.append(revcomp(r) if rc and rng.random() < 0.5 else r)
    return out


def random_case(seed=1, genome_len=3000, n_reads=300, lens=(40, 63, 64, 65, 100, 129, 150, 200), n_queries=60, err=0.02):
    """a few hundred error-free reads of mixed lengths on both strands, and queries: some of the reads with substitutions,
    some fresh pieces of the genome that are not in the index, some with an N"""
    g = random_genome(genome_len, seed)
    refs = sample_reads(g, n_reads, lens, seed + 1)
    rng = random.Random(seed + 2)
    queries = []
    for i in range(n_queries):
        if i % 3 == 0:
            q = refs[rng.randrange(len(refs))]
        else:
            L = rng.choice(lens)
            o = rng.randrange(0, genome_len - L + 1)
            q = g[o:o + L]
            if rng.random() < 0.5:
                q = revcomp(q)
        pos = [x for x in range(len(q)) if rng.random() < err]
        q = mutate(q, pos)
        if i % 7 == 3:
            x = rng.randrange(len(q))
            q = q[:x] + "N" + q[x + 1:]
        queries.append(q)
    return dict(genome=g, refs=refs, queries=queries)


def seedable_case(seed=5):
    """reads and queries where every acceptable alignment holds an error-free seed: few, widely spaced substitutions, a short
    seed at stride 1, and an overlap floor that is longer than the longest stretch between two substitutions needs"""
    g = random_genome(600, seed)
    refs = sample_reads(g, 40, (50, 70, 90), seed + 1)
    rng = random.Random(seed + 2)
    queries = []
    for i in range(8):
        L = (60, 80)[i % 2]
        o = rng.randrange(0, len(g) - L + 1)
        q = g[o:o + L]
        if i % 2:
            q = revcomp(q)
        queries.append(mutate(q, [10, 45] if i % 3 else []))
    # S = 12, T = 1: a window of 12 at every place.  The reads are error-free, so an alignment in place sees at most the
    # query's substitutions at columns 10 and 45, and any stretch of M = 40 columns holds 12 clean ones in a row beside
    # them (at worst columns 11 .. 44 or 46 .. 59); an alignment out of place has some 3/4 of its columns wrong and is refused
    return dict(refs=refs, queries=queries, params=params(S=12, T=1, M=40, P=50, H=4096, K=4096))


def second_round_case():
    """P = 25: an overlap of 80 to 119 columns may hold 2 mismatches.  The query has two substitutions near its start and one
    near its end.  Six reads over its first 80-odd columns see the two, are accepted and repair them.  Six reads over the whole
    query see three mismatches and are refused in round 1.  Two reads over the end carry the query's own base at the third place:
    they keep the read valid (D = 2) but are fewer than C = 5.  In round 2 the six whole reads see one mismatch, are accepted and
    outvote the two."""
    g = random_genome(600, 21)
    truth = g[200:300]
    q = mutate(truth, [5, 12, 95])
    gm = mutate(g, [295])
    left = [g[150 - i:280 + i // 2] for i in range(0, 12, 2)]
    whole = [g[196 - i:304 + i] for i in range(1, 7)]
    right = [gm[240 + i:340 + i] for i in range(0, 2)]
    return dict(refs=left + whole + right, queries=[q], truth=truth, params=params(S=24, T=12, M=45, P=25, C=5, D=2))
