#!/usr/bin/env python3
"""Writes the fixtures of tests/test_lca.py under tests/golden/lca/:
  names.dmp          a synthetic names.dmp over tests/golden/analysis/nodes.dmp ("Taxon <taxid>" as the scientific name of every
                     taxid, a synonym line in front of every tenth one, which a reader must skip)
  small_nodes.dmp    a hand-built tree with every rank code of the report (R, R1, D twice: superkingdom and domain, K, P, C, O, F,
                     G, S, S1, S2), a tie in clade_reads between two species, and an unrooted chain (30 -> 31 -> 40, 40 unlisted)
  small_names.dmp    its names (taxid 8 has none: the report prints the number)
  small_rows.tsv     hand-filled rows: taxid, clade_reads, direct_reads
  small_report_names.txt / small_report_plain.txt / small_report_all_classified.txt
                     the expected reports, typed in by hand below (100 reads of which 90 classified, with and without names; and
                     the same rows with reads = classified = 90), not produced by any code under test
usage: tests/golden/make_lca_golden.py"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "lca")

NODE_LINE = "%d\t|\t%d\t|\t%s\t|\t\t|\t0\t|\t1\t|\t11\t|\t1\t|\t0\t|\t1\t|\t0\t|\t0\t|\t\t|\n"
SMALL = [(1, 1, "no rank"), (2, 1, "superkingdom"), (3, 1, "no rank"), (4, 3, "domain"), (5, 4, "kingdom"), (6, 5, "phylum"), (7, 6, "class"),
         (8, 7, "order"), (9, 8, "family"), (10, 9, "genus"), (11, 10, "species"), (12, 11, "strain"), (13, 12, "no rank"), (14, 10, "species"),
         (15, 2, "species"), (30, 31, "species"), (31, 40, "genus")]
SMALL_NAMES = {1: "root", 2: "Bacteria", 3: "cellular organisms", 4: "Domain four", 5: "Kingdom five", 6: "Phylum six", 7: "Class seven",
               9: "Family nine", 10: "Genus ten", 11: "Species eleven", 12: "Strain twelve", 13: "Isolate thirteen", 14: "Species fourteen",
               15: "Species fifteen"}
# taxid, clade, direct: 90 classified reads
ROWS = [(1, 90, 2), (2, 50, 30), (3, 38, 7), (4, 31, 6), (5, 25, 0), (6, 25, 0), (7, 25, 0), (8, 25, 0), (9, 25, 1), (10, 24, 4), (11, 10, 2),
        (12, 8, 3), (13, 5, 5), (14, 10, 10), (15, 20, 20)]
# the report's lines in order: share of 100 reads, share of 90 reads, clade, direct, code, taxid, depth
LINES = [(" 90.00", "100.00", 90, 2, "R", 1, 0), (" 50.00", " 55.56", 50, 30, "D", 2, 1), (" 20.00", " 22.22", 20, 20, "S", 15, 2),
         (" 38.00", " 42.22", 38, 7, "R1", 3, 1), (" 31.00", " 34.44", 31, 6, "D", 4, 2), (" 25.00", " 27.78", 25, 0, "K", 5, 3),
         (" 25.00", " 27.78", 25, 0, "P", 6, 4), (" 25.00", " 27.78", 25, 0, "C", 7, 5), (" 25.00", " 27.78", 25, 0, "O", 8, 6),
         (" 25.00", " 27.78", 25, 1, "F", 9, 7), (" 24.00", " 26.67", 24, 4, "G", 10, 8), (" 10.00", " 11.11", 10, 2, "S", 11, 9),
         ("  8.00", "  8.89", 8, 3, "S1", 12, 10), ("  5.00", "  5.56", 5, 5, "S2", 13, 11), (" 10.00", " 11.11", 10, 10, "S", 14, 9)]


def report(col, names, unclassified):
    out = [" 10.00\t10\t10\tU\t0\tunclassified\n"] if unclassified else []
    for ln in LINES:
        out.append("%s\t%d\t%d\t%s\t%d\t%s%s\n" % (ln[col], ln[2], ln[3], ln[4], ln[5], "  " * ln[6], names.get(ln[5], str(ln[5]))))
    return "".join(out)


def main():
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "names.dmp"), "w") as f:
        for k, line in enumerate(open(os.path.join(HERE, "analysis", "nodes.dmp"))):
            t = int(line.split("|")[0])
            if k % 10 == 0:
                f.write("%d\t|\tOld name of %d\t|\t\t|\tsynonym\t|\n" % (t, t))
            f.write("%d\t|\tTaxon %d\t|\t\t|\tscientific name\t|\n" % (t, t))
    with open(os.path.join(OUT, "small_nodes.dmp"), "w") as f:
        for t, p, r in SMALL:
            f.write(NODE_LINE % (t, p, r))
    with open(os.path.join(OUT, "small_names.dmp"), "w") as f:
        for t in sorted(SMALL_NAMES):
            f.write("%d\t|\tcommon name of %d\t|\t\t|\tgenbank common name\t|\n" % (t, t))
            f.write("%d\t|\t%s\t|\t\t|\tscientific name\t|\n" % (t, SMALL_NAMES[t]))
    with open(os.path.join(OUT, "small_rows.tsv"), "w") as f:
        for r in ROWS:
            f.write("%d\t%d\t%d\n" % r)
    open(os.path.join(OUT, "small_report_names.txt"), "w").write(report(0, SMALL_NAMES, True))
    open(os.path.join(OUT, "small_report_plain.txt"), "w").write(report(0, {}, True))
    open(os.path.join(OUT, "small_report_all_classified.txt"), "w").write(report(1, SMALL_NAMES, False))


if __name__ == "__main__":
    main()
