#!/usr/bin/env python3
"""Regenerates every golden vector under tests/golden/ from the UNMODIFIED reference.

Needs oracle/_ref (built by `make -C oracle ref` in the container that has
/root/reference).  Everything written here is DATA: synthetic inputs plus the outputs the
compiled reference produced for them (strict build: -ffp-contract=off).

  tables.bin            fmath expd/log tables + probe values      (ref_harness tables)
  corpus.fa/.racc       Raccess acc/cond for an edge-case corpus   (ref_harness raccess)
  c1_{q,db}.fa          BASELINE config 1 inputs (32x200 vs 32x200, seeds 2/1)
  c1db.*.gz             the reference `db` output for c1_db.fa (defaults)
  c1_ris_s{0,1}.out     reference `ris` output (-s 0 / -s 1), body lines sorted, Id stripped
  c1.stg.gz             per-stage hit dumps for C1                 (ref_harness stages)
  mix_*.fa, mixdb.*.gz, mix_ris_s{0,1}.out, mix.stg.gz
                        mixed-length case: N / lowercase, 3 DB pages (-c 10)
  c1_q.sa               encoder + suffix array goldens             (ref_harness sa)
  widew.fa, widew_w<W>d<delta>.racc
                        Raccess beyond the default band: maximal spans 100, 129, 150 and 200 (spans wider than
                        the 64 / 128 cells the HIP kernels' default mappings cover), several window lengths
  quirk_*.fa, quirkdb.*.gz, quirk_ris_s{0,1}.out, quirk.stg.gz
                        designed duplexes with a bulge next to the seed: the FIRST post-ungapped hit of a
                        query is gapped-extended and survives the final filter, so it keeps the unsorted
                        base-pair order of rna_interaction_search.cpp:314-317; 5 DB pages
  edge_*.fa, edgedb.*.gz, edge_ris_s{0,1}.out, edge.stg.gz
                        the database side at its edges (edge_inputs): targets of 4 to 33 nt next to each other,
                        targets that are nothing but a site, trap neighbours behind the separators, sites at text
                        position 0 and nchars - 1, a page of one sequence; 5 DB pages (-c 8).
                        `make_golden.py edge` regenerates this case alone
  mix_opt<k>.stg.gz     the `mix` case's stage dumps under the non-default `ris` options of tests/option_sets.py
                        (OPTION_SETS[k]); a set that changes neither -l nor -e has the seed lists of mix.stg - checked
                        here, record for record - and is stored with empty seed lists.  `make_golden.py mixopt`
  widew_short.fa        the sequences of widew.fa of at most 700 nt, for the span 255 (widew_w255d2.racc)
"""
import gzip
import os
import random
import shutil
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_synthetic  # noqa: E402
import option_sets  # noqa: E402


def run(*cmd, cwd=None):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    subprocess.run(list(cmd), check=True, cwd=cwd, env=env)


def gz(src, dst):
    with open(src, "rb") as f, gzip.GzipFile(dst, "wb", mtime=0) as g:
        shutil.copyfileobj(f, g)


def body_sorted(path):
    with open(path) as f:
        lines = f.read().splitlines()
    head, body = lines[:3], lines[3:]
    body = sorted(l.split(",", 1)[1] for l in body)
    return head, body


def corpus():
    rng = random.Random(7)
    recs = []
    for L in range(1, 11):
        recs.append((f"len{L}", "".join(rng.choice("ACGU") for _ in range(L))))
    recs.append(("len60", "".join(rng.choice("ACGU") for _ in range(60))))
    recs.append(("len71", "".join(rng.choice("ACGU") for _ in range(71))))
    recs.append(("len72", "".join(rng.choice("ACGU") for _ in range(72))))
    recs.append(("len200", "".join(rng.choice("ACGU") for _ in range(200))))
    recs.append(("len330", "".join(rng.choice("ACGU") for _ in range(330))))
    recs.append(("len1000", "".join(rng.choice("ACGU") for _ in range(1000))))
    recs.append(("gc2000", "".join(rng.choice("GGGCCCAU") for _ in range(2000))))
    recs.append(("len2700", "".join(rng.choice("ACGU") for _ in range(2700))))
    recs.append(("polyA", "A" * 90))
    recs.append(("polyGC", "GC" * 60))
    recs.append(("hairpins", ("GGGGGCCAAAAGGCCCCC" + "AUAU") * 8))
    s = list("".join(rng.choice("ACGU") for _ in range(300)))
    for k in range(100, 120):
        s[k] = "N"
    for k in range(200, 240):
        s[k] = s[k].lower()
    recs.append(("withN_lower", "".join(s)))
    recs.append(("dna_T", "".join(rng.choice("ACGT") for _ in range(150))))
    recs.append(("allN", "N" * 40))
    return recs


WIDE_W = [(100, 5), (129, 5), (129, 2), (150, 5), (200, 4)]
# the spans at which the HIP kernels change form: 64 / 65 cells per pass, 96 / 97 for the row masks, 127 / 128 for the
# two-pass mapping, and the limit 255 - the last on the sequences of at most WIDE_SHORT nt (widew_short.fa)
EDGE_W = [(64, 5), (65, 5), (96, 5), (97, 5), (128, 5)]
LIMIT_W = (255, 2)
WIDE_SHORT = 700


def widew_corpus():
    """A subset of corpus() (same sequences: same generator, same order) + one GC-rich 700-mer whose log Z sits in
    the linear bulge / interior branch at every span."""
    d = dict(corpus())
    recs = [(k, d[k]) for k in ("len4", "len60", "len72", "len200", "len330", "len1000", "hairpins", "withN_lower", "polyGC")]
    rng = random.Random(17)
    recs.append(("len150", "".join(rng.choice("ACGU") for _ in range(150))))
    recs.append(("gc700", "".join(rng.choice("GGGCCCAU") for _ in range(700))))
    recs.append(("gc1500", "".join(rng.choice("GGGCCCAU") for _ in range(1500))))
    return recs


def mix_inputs():
    rng = random.Random(11)
    db = []
    for i in range(24):
        L = rng.randint(50, 400)
        s = list("".join(rng.choice("ACGU") for _ in range(L)))
        if i % 5 == 0:
            a = rng.randint(0, L - 12)
            for k in range(a, a + 10):
                s[k] = "N"
        if i % 7 == 0:
            a = rng.randint(0, L - 20)
            for k in range(a, a + 18):
                s[k] = s[k].lower()
        db.append((f"mdb{i}", "".join(s)))
    q = []
    for i in range(6):
        L = rng.randint(100, 600)
        s = list("".join(rng.choice("ACGU") for _ in range(L)))
        if i == 2:
            for k in range(40, 46):
                s[k] = "N"
        q.append((f"mq{i}", "".join(s)))
    # one query that is the reverse complement of a DB stretch: long perfect duplex
    comp = {"A": "U", "C": "G", "G": "C", "U": "A"}
    src = db[3][1][20:90].upper().replace("N", "A")
    q.append(("mq_rc", "ACGUACGUAC" + "".join(comp[c] for c in reversed(src)) + "UUGACCA"))
    return q, db


def quirk_inputs():
    """Queries X+Y (or Y+X) in poly-A, targets rc(Y)+bulge+rc(X) in poly-C: the seed covers one arm, the
    ungapped extension stops at the bulge, the gapped extension crosses it.  The designs (seeds 1, 2, 3, 5, 8 of
    the generator below) were picked with `ref_harness stages`: each gives a final hit whose stored pairs are
    [diagonal, left chain, right chain outer->inner], i.e. not ascending."""
    comp = {"A": "U", "C": "G", "G": "C", "U": "A"}

    def rc(x):
        return "".join(comp[c] for c in reversed(x))
    q, db = [], []
    for k, seed in enumerate((1, 2, 3, 5, 8)):
        rng = random.Random(seed)
        X = "".join(rng.choice("GC" if rng.random() < 0.6 else "AU") for _ in range(rng.randint(8, 12)))
        Y = "".join(rng.choice("GC" if rng.random() < 0.6 else "AU") for _ in range(rng.randint(5, 9)))
        bulge = "".join(rng.choice("AC") for _ in range(rng.randint(1, 2)))
        side = rng.random() < 0.5
        q.append((f"kq{k}", "A" * 25 + (X + Y if side else Y + X) + "A" * 25))
        db.append((f"kd{k}", "C" * 20 + (rc(Y) + bulge + rc(X) if side else rc(X) + bulge + rc(Y)) + "C" * 20))
        db.append((f"kdecoy{k}", "".join(rng.choice("ACGU") for _ in range(120))))
    rng = random.Random(99)
    q.append(("kq_random", "".join(rng.choice("ACGU") for _ in range(150))))
    return q, db


# (no 1, 2 or 3 nt: `db` stores L - 4 as a target's count of accessibilities, and the reference's `ris` aborts on a
# negative count when it loads the database - DESIGN.md 2)
EDGE_TINY = (4, 5, 7, 8, 9, 20, 31, 32, 33)
EDGE_PAGE = 8  # `db -c`: sequences per page


def edge_inputs():
    """Database side at its edges (33 targets, pages of 8: 5 pages, the last of one sequence).  The page text holds the
    targets reversed and 0-terminated in file order, so file neighbours are text neighbours.

      page 0  site-only targets (nothing but rc(a query stretch): the hit spans the sequence) as the first and the last
              sequence of the page, and two more between TRAP neighbours - tiny targets whose bases continue the
              complement behind the separator, once on the diagonal (one query base skipped: a 1x1 loop for an
              extension that steps over the separator), once next to it (a 1-nt bulge)
      page 1  quirk-style designs rc(Y)+bulge+rc(X) with the poly-C flank on one side only (one per side), two
              identical targets next to each other, an all-N and an all-lower-case target, a 20-nt site-only target
      page 2  only targets too short to be hit: eight of 4 nt - seven starts in the first 32-character block
      page 3  5, 7, 8, 9, 31, 32, 33 nt and a site-only target
      page 4  one site-only target: text position 0 and nchars - 1 belong to the same hit
    Queries: stretches at position 0 and at the last base, a query that is only a site (shorter than the
    accessibility span, and the second query on that target), a random 150-mer, three degenerate strings."""
    comp = {"A": "U", "C": "G", "G": "C", "U": "A"}

    def rc(x):
        return "".join(comp[c] for c in reversed(x))
    rng = random.Random(2024)

    def rnd(n, alphabet="ACGU"):
        return "".join(rng.choice(alphabet) for _ in range(n))

    def site(n):
        return "".join(rng.choice("GC" if rng.random() < 0.65 else "AU") for _ in range(n))
    A, Z, B, C, E, F, G20 = site(16), site(15), site(14), site(18), site(12), site(17), site(20)
    p1, n1, p2, n2 = site(5), site(7), site(4), site(5)
    p1, n1, p2, n2 = "GC" + p1[2:], n1[:-2] + "CG", "CG" + p2[2:], n2[:-2] + "GC"
    q, db = [], []
    q.append(("eq_ends", A + rnd(20, "AU") + G20 + rnd(20, "AU") + Z))        # sites at position 0 and at the last base
    q.append(("eq_trap1", rnd(12, "AU") + p1 + "A" + B + "A" + n1 + rnd(12, "AU")))  # traps on the diagonal
    q.append(("eq_trap2", rnd(12, "AU") + p2 + C + n2 + rnd(9, "AU") + E + rnd(7, "AU") + F))  # traps beside it
    q.append(("eq_site", B))                                                   # nothing but a site
    rnd150 = rnd(150)
    kq, kdb = [], []
    for k, (seed, end) in enumerate(((1, "l"), (2, "r"), (5, "l"))):
        r2 = random.Random(seed)
        X = "".join(r2.choice("GC" if r2.random() < 0.6 else "AU") for _ in range(r2.randint(8, 12)))
        Y = "".join(r2.choice("GC" if r2.random() < 0.6 else "AU") for _ in range(r2.randint(5, 9)))
        bulge = "".join(r2.choice("AC") for _ in range(r2.randint(1, 2)))
        side = r2.random() < 0.5
        kq.append((f"eq_k{k}", "A" * 25 + (X + Y if side else Y + X) + "A" * 25))
        core = rc(Y) + bulge + rc(X) if side else rc(X) + bulge + rc(Y)
        kdb.append((f"ed_k{k}{end}", core + "C" * 20 if end == "l" else "C" * 20 + core))
    q += kq
    q.append(("eq_random", rnd150))
    q += [("eq_deg_n", "N" * 40), ("eq_deg_gc", "GC" * 40), ("eq_deg_acgu", "ACGU")]
    # page 0
    db += [("ed_first", rc(A)), ("ed_p1", rc(p1)), ("ed_trap1", rc(B)), ("ed_n1", rc(n1)),
           ("ed_p2", rc(p2)), ("ed_trap2", rc(C)), ("ed_n2", rc(n2)), ("ed_last", rc(Z))]
    # page 1
    twin = rnd(9) + rc(rnd150[40:58]) + rnd(6)
    db += kdb[:2] + [("ed_twin_a", twin), ("ed_twin_b", twin), ("ed_alln", "N" * 7),
                     ("ed_lower", (rnd(5) + rc(Z) + rnd(4)).lower()), ("ed_site20", rc(G20)), kdb[2]]
    # page 2: too short for a seed
    db += [(f"ed_tiny{k}", rnd(4)) for k in range(EDGE_PAGE)]
    # page 3
    db += [(f"ed_len{n}", rnd(n)) for n in (5, 7, 8, 9, 31, 32, 33)] + [("ed_site12", rc(E))]
    # page 4
    db.append(("ed_alone", rc(F)))
    assert len(db) == 4 * EDGE_PAGE + 1 and sum(len(s) for _, s in db) < 2000
    assert set(EDGE_TINY) <= {len(s) for _, s in db}
    return q, db


def main():
    assert os.path.exists(os.path.join(REF, "ref_harness")), "run `make -C oracle ref` first"
    strict = os.path.join(REF, "pRIblast.strict")
    harness = os.path.join(REF, "ref_harness")
    tmp = tempfile.mkdtemp(prefix="golden_")
    only = set(sys.argv[1:])  # e.g. `make_golden.py quirk`: only the ris cases named

    if not only:
        run(harness, "tables", os.path.join(HERE, "tables.bin"))

        gen_synthetic.write_fasta(os.path.join(HERE, "corpus.fa"), corpus())
        run(harness, "raccess", os.path.join(HERE, "corpus.fa"), "70", "5", os.path.join(HERE, "corpus.racc"))

        # ---- config 1 ----
        gen_synthetic.write_fasta(os.path.join(HERE, "c1_db.fa"), gen_synthetic.gen(32, 200, 1, "db"))
        gen_synthetic.write_fasta(os.path.join(HERE, "c1_q.fa"), gen_synthetic.gen(32, 200, 2, "q"))
        # a second (W, delta) so the band geometry is not hard-wired to the defaults
        run(harness, "raccess", os.path.join(HERE, "c1_q.fa"), "40", "7", os.path.join(HERE, "c1_q_w40d7.racc"))
        run(harness, "sa", os.path.join(HERE, "c1_q.fa"), "0", os.path.join(HERE, "c1_q.sa"))
    if not only or "widew" in only:
        gen_synthetic.write_fasta(os.path.join(HERE, "widew.fa"), widew_corpus())
        for W, delta in WIDE_W + EDGE_W:
            run(harness, "raccess", os.path.join(HERE, "widew.fa"), str(W), str(delta),
                os.path.join(HERE, f"widew_w{W}d{delta}.racc"))
        gen_synthetic.write_fasta(os.path.join(HERE, "widew_short.fa"), [r for r in widew_corpus() if len(r[1]) <= WIDE_SHORT])
        run(harness, "raccess", os.path.join(HERE, "widew_short.fa"), str(LIMIT_W[0]), str(LIMIT_W[1]),
            os.path.join(HERE, "widew_w%dd%d.racc" % LIMIT_W))
    cases = [("c1", "c1_q.fa", "c1_db.fa", []), ("mix", "mix_q.fa", "mix_db.fa", ["-c", "10"]),
             ("quirk", "quirk_q.fa", "quirk_db.fa", ["-c", "2"]),
             ("edge", "edge_q.fa", "edge_db.fa", ["-c", str(EDGE_PAGE)])]
    if only:
        cases = [c for c in cases if c[0] in only]
    mq, mdb = mix_inputs()
    gen_synthetic.write_fasta(os.path.join(HERE, "mix_q.fa"), mq)
    gen_synthetic.write_fasta(os.path.join(HERE, "mix_db.fa"), mdb)
    kq, kdb = quirk_inputs()
    gen_synthetic.write_fasta(os.path.join(HERE, "quirk_q.fa"), kq)
    gen_synthetic.write_fasta(os.path.join(HERE, "quirk_db.fa"), kdb)
    eq, edb = edge_inputs()
    gen_synthetic.write_fasta(os.path.join(HERE, "edge_q.fa"), eq)
    gen_synthetic.write_fasta(os.path.join(HERE, "edge_db.fa"), edb)
    for tag, qfa, dbfa, dbopts in cases:
        dbp = os.path.join(tmp, tag + "db")
        run(strict, "db", "-i", os.path.join(HERE, dbfa), "-o", dbp, *dbopts, cwd=tmp)
        for ext in ("bas", "seq", "acc", "nam", "ind"):
            gz(f"{dbp}.{ext}", os.path.join(HERE, f"{tag}db.{ext}.gz"))
        for style in (0, 1):
            out = os.path.join(tmp, f"{tag}_s{style}.out")
            run(strict, "ris", "-i", os.path.join(HERE, qfa), "-o", out, "-d", dbp, "-s", str(style), cwd=tmp)
            head, body = body_sorted(out)
            with open(os.path.join(HERE, f"{tag}_ris_s{style}.out"), "w") as f:
                f.write("\n".join(head[:1] + head[2:] + body) + "\n")
        stg = os.path.join(tmp, tag + ".stg")
        run(harness, "stages", os.path.join(HERE, qfa), dbp, stg)
        gz(stg, os.path.join(HERE, tag + ".stg.gz"))
    if not only or "mixopt" in only:
        mixopt(strict, harness, tmp)
    shutil.rmtree(tmp)


def mixopt(strict, harness, tmp):
    """mix_opt<k>.stg.gz for every set of option_sets.OPTION_SETS."""
    import refdump
    dbp = os.path.join(tmp, "mixdb")
    if not os.path.exists(dbp + ".bas"):
        run(strict, "db", "-i", os.path.join(HERE, "mix_db.fa"), "-o", dbp, "-c", "10", cwd=tmp)
    nq = len(mix_inputs()[0])
    base = os.path.join(tmp, "mix_default.stg")
    run(harness, "stages", os.path.join(HERE, "mix_q.fa"), dbp, base)
    with gzip.open(os.path.join(HERE, "mix.stg.gz"), "rb") as f, open(base, "rb") as g:
        assert f.read() == g.read(), "mix.stg.gz is stale: regenerate the mix case first"
    default = refdump.read_stages(base)

    def flat(h):
        return tuple(h[k] for k in ("q_sp", "db_sp", "q_len", "db_len", "db_id", "db_id_start")) + tuple(
            struct.pack("<d", h[k]) for k in ("e_acc", "e_hyb", "e_tot")) + (h["bp"].tobytes(),)
    for k, kw in enumerate(option_sets.OPTION_SETS):
        stg = os.path.join(tmp, f"mix_opt{k}.stg")
        run(harness, "stages", os.path.join(HERE, "mix_q.fa"), dbp, stg, *option_sets.switches(kw))
        recs = refdump.read_stages(stg)
        assert len(recs) == len(default) and len(recs) % nq == 0
        if not option_sets.holds_seeds(k):
            for a, b in zip(recs, default):
                assert (a["q"], a["page"]) == (b["q"], b["page"])
                assert [flat(h) for h in a["seed"]] == [flat(h) for h in b["seed"]], (k, a["q"], a["page"])
            refdump.write_stages(stg, nq, len(recs) // nq, recs, keep_seeds=False)
        gz(stg, os.path.join(HERE, option_sets.fixture(k)))
        n = [sum(len(r[s]) for r in recs) for s in ("seed", "ungapped", "gapped")]
        print(f"mix_opt{k} {kw}: seed {n[0]} ungapped {n[1]} gapped {n[2]}, "
              f"{os.path.getsize(os.path.join(HERE, option_sets.fixture(k)))} bytes")


if __name__ == "__main__":
    main()
