// pRIblast-hip: drop-in for the reference's `ris` sub-command on top of the C ABI.
//
// Command line, defaults, error texts and the output format follow the reference
// (main.cpp:36-111, 148-175; rna_interaction_search_parameters.cpp:33-114;
// rna_interaction_search.cpp:322-369, 445-476).  `-a` is accepted and ignored: the MPI/OpenMP query
// schedulers are replaced by batched GPU stages.  Queries are sorted by length, longest first, as the
// reference does before dealing them (utils.cpp:56-63, rna_interaction_search.cpp:145-153), cut into
// batches of PRB_BATCH, and
//   * one process: dealt from a counter to the workers named by PRB_DEVICES (default: device 0), one
//     host thread each; a worker computes the accessibilities of its next batch under a second
//     context while the current batch is searched; one writer thread prints finished batches in order;
//     With fewer batches than workers (one lncRNA against a transcriptome) and a database of several pages
//     (`db -c`), the workers share each batch instead (PRB_SPLIT): everyone takes pages of it from a counter, and
//     the first worker merges the others' tables into its own on the device (prb_*_merge) - run_team;
//   * one process per GPU (WORLD_SIZE / RANK / LOCAL_RANK in the environment, as torchrun or mpirun
//     set them): batch b goes to rank b mod WORLD_SIZE, and after every round of batches the final
//     hits are gathered on rank 0 over RCCL (prb_gather_hits), which writes the lines - the
//     replacement of the reference's MPI token ring (rna_interaction_search.cpp:426-487).  The 128-byte
//     RCCL id travels through a file in the `-p` temporary directory (default: next to the output).
//
// Three additions to the reference's surface (the output path): `ris -b` writes
// the hits as binary records instead of text (no number formatting on the search path), the
// `txt` sub-command turns such a file into exactly the text `ris` would have written, and `ris -t`
// writes one summary line per (query, target) pair instead of one line per hit: the final hits are
// reduced on the GPU (prb_search_page_summary) and never leave it.  `-t` is refused with `-b` and in
// rank mode (WORLD_SIZE > 1): the gather carries hit records only.  `-t -n N` keeps each query's N
// pairs of lowest minimum energy: a table on the GPU (prb_search_page_top) takes every page of a
// batch, and only its N records per query reach the host.  `ris -q` writes one line per query position
// that a final hit covers (hits, distinct targets, minimum energy and its first hit): a per-position
// table on the GPU (prb_search_page_profile) takes every page of a batch, and only its covered rows
// reach the host.  `-q` is refused with -t, -n, -b and in rank mode, as -t is.  `ris -k N` writes the normal result
// lines (or, with -b, the normal binary records) of each query's N final hits of lowest interaction energy only, best
// first: a table on the GPU (prb_search_page_tophits) takes every page of a batch and keeps those hits with their base
// pairs, and only they reach the host.  `-k` is refused with -t, -n, -q and in rank mode.  `ris -u` keeps only the distinct
// interaction sites of each (query, target) pair - greedy non-maximum suppression on the GPU, before the traceback
// (prb_ris_opts::distinct_sites) - and combines with every mode: each of them takes the thinned list.  `ris -j` keeps each
// pair's best co-linear chain of sites instead - the sites that can bind at the same time, by a dynamic programme on the
// GPU at the same point (prb_ris_opts::chain_sites); it combines like -u and is refused with it.  `ris -r N` turns
// `-t -n` round: the `-t` lines of each TARGET's N pairs of lowest minimum energy over all the queries of the run.  Every
// worker owns one table on its GPU for the whole run (prb_search_page_targets takes every page of every batch it
// searches); at the end the first worker merges the others' into its own (prb_targetset_merge), and only N records per
// target reach the host, written by page, target and rank.  `-r` is refused with -t, -n, -q, -k, -b and in rank mode.
// `ris -t -z N` adds an empirical p-value to every `-t` line: N shuffled decoys of each query (prb_shuffle_sequence) are
// searched like the query, and a null table on the GPU (prb_nullset_*) counts, per observed pair, the decoys that reach
// its minimum energy; only the table's records reach the host.  `-z` needs -t and is refused with -n, -k, -q, -r, -c, -b.
// `ris -c D` says where on a target the queries bind: one line per region - a maximal run of positions of one database
// sequence, each covered by final hits of at least D distinct queries.  Every worker owns one per-position table of the
// database on its GPU for the whole run (prb_search_page_coverage takes every page of every batch it searches); at the
// end the first worker merges the others' into its own (prb_covset_merge), the regions are reduced on the device
// (prb_covset_finish) and only their records reach the host, written by page, target and start.  `-c` is refused with
// -t, -n, -q, -k, -b, -r and in rank mode; -u and -j combine.
// `ris -t -G FILE -P N` adds an empirical p-value to every `-t -G [-n K]` line: the decoys of `-z`, but counted per group -
// a decoy's minimum over all members of the group against the group's minimum - in a group null table on the GPU
// (prb_gnullset_*), the decoys searched against the members of each query's kept groups only.  `-P` needs -G and is
// refused with -z, -k, -q, -r, -c, -b and in rank mode.
// `ris -k K -E M` scores every `-k` line: the real batch is searched once into the top-N hit table and - the same
// sub-batches - into an evalset on the GPU (prb_search_page_scored), then M shuffled decoys of each query against the whole
// database (prb_search_page_null_hits: only their hits' energy keys are kept); the evalset is closed and the kept hits
// looked up in it (prb_evalset_score).  `-E` needs -k and is refused with -b, -t, -n, -q, -r, -c, -z, -G, -P and in rank mode.
// `ris -t -G FILE -R N` is `-r` at the level of the groups: the `-t -G` lines of each GROUP's N queries of lowest minimum
// energy over all the queries of the run.  A group's members may lie on any page, so a batch is searched against every
// page into its group table as for `-t -G` (with PRB_SPLIT the workers' tables merged), and that table - complete, never
// copied to the host - is merged on the device into the group ranking table that the worker owns for the whole run
// (prb_grouprank_add_groupset, under the queries' input positions); at the end the first worker merges the others' into
// its own (prb_grouprank_merge), and only N records per group reach the host, written by group and rank.  `-R` needs -G
// and is refused with -n and -P; everything else is refused through -G.
//
// `ris -t -A FILE` is `-t` one level below the target: a line per (query, annotated feature of a target) over the final
// hits whose span meets the feature.  The annotation is read and checked before any GPU work (load_features), uploaded
// once per worker (prb_annot_create, open_workers), and a batch's pages are folded into its feature table on the device
// (prb_search_page_features; with PRB_SPLIT the workers' tables merged, prb_featset_merge): only the records reach the host.
// `ris -t -A FILE -F N` adds an empirical p-value to every `-t -A` line: the decoys of `-z`, but counted per feature - a
// decoy's minimum over its hits that meet the feature against the feature's minimum - in a feature null table on the GPU
// (prb_fnullset_*), the decoys searched against the targets of each query's kept records only.  `-F` needs -A and is
// refused with what -A is refused with, and in rank mode.
// `ris -t -A FILE -N K` keeps each query's K records of lowest minimum energy (ties in -t -A order), best first: the cut
// is made on the device when the batch's feature table is finished (prb_featset_finish_top), so only K records per query
// reach the host, and the lines are lines of the `-t -A` run.  With -F the feature null table is made over the cut
// (prb_fnullset_create_top): its lookup and scratch hold the kept records only, and a query's decoys are searched against
// the targets of its K kept records only.  `-N` needs -A; everything else is refused through -A.
// `ris -t -A FILE -B N` is `-R` at the level of the features: the `-t -A` lines of each FEATURE's N queries of lowest
// minimum energy over all the queries of the run.  A batch is searched page by page into its feature table as for `-t -A`
// (with PRB_SPLIT the workers' tables merged), and that table - complete, never finished, never copied to the host - is
// merged on the device into the feature ranking table that the worker owns for the whole run (prb_featrank_add_featset,
// under the queries' input positions); at the end the first worker merges the others' into its own (prb_featrank_merge),
// and only N records per feature reach the host, written by feature - in the order load_features numbers them - and rank.
// `-B` needs -A and is refused with -F and -N; everything else is refused through -A.
//
// `ris -t -z N -H H [-D R]` makes the p-values of -z sequential: the decoys are searched in rounds of R, and at every round's
// end the null table retires, on the device, the pairs that H or more of their decoys have reached (prb_nullset_retire);
// the next round's pieces are searched under a mask of the pairs still live, made on the device from the table
// (prb_pairmask_create_live), and a query without live pairs gets no further decoys.  No record reaches the host between
// rounds.  `-H` needs -z, `-D` needs -H.
//
// `ris -t -z N -Q [-H H [-D R]]` puts a Benjamini-Hochberg q-value behind every -z line: the null table is finished with
// prb_nullset_finish_fdr, which ranks each query's p-values on the device as exact fractions and takes the step-up
// minimum there (finish_null_table); the records and their order are those of the run without -Q, and three columns
// follow them: Tests - the targets the query was searched against, under -L the distinct targets listed for it -,
// Rank and QValue.  `-Q` takes no argument and needs -z.
//
// How the file is laid out.  The switches -t -n -q -k -b -u -j -r -c -z -Z -G -P -E -R -A -F -N -B -H -D -Q have one table (kSwitchTable) that every
// refusal is generated from, and decide one OutputMode.  ris_main is a sequence of steps over one Run: parse_args (then
// load_pairlist, load_groups and load_features, which read the files of -L, -G and -A), rank_setup, open_workers, join_ranks (the
// Rendezvous), read_seq_tables, open_output (header_text), plan_batches, then run_workers or run_ranks (the Gatherer), and
// close_run.  The producers (run_workers' two forms, run_ranks) drive run_batches, whose search_batch returns a
// BatchResult - the one owner of whatever handles a mode leaves - and hand it as a BatchJob to the Writer, whose thread
// calls write_job.  search_batch has two shapes.  Most modes: create_table, search_one_page for every page, finish_table
// - the three steps that a team of workers shares out (Team::search).  The modes with decoys (runs_decoys: -z, -P, -E, -F)
// have a function each that makes, fills and finishes its own tables around one loop, for_decoy_pieces: it cuts the
// batch's decoys into pieces, shuffles them, makes each piece's query batch and hands it as a DecoyPiece to the mode's
// body, which decides the piece's mask (mask_piece, mask_piece_by_list) and searches the pages.  Free has a deleter for
// every handle of the C ABI that this file keeps in a Handle.
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <numeric>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <cctype>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/priblast_hip.h"
#include "db_format.hpp"
#include "fasta.hpp"
#include "output.hpp"

namespace {

using prb::BatchView;
using prb::LineSink;
using prb::PageHits;
using prb::SeqTable;

void usage() {
  std::puts("pRIblast-hip - RNA-RNA interaction search (ris step of pRIblast) on AMD Instinct GPUs\n"
            "\n"
            "pRIblast-hip ris -i InputFastaFile -o OutputFileName -d DatabaseFileName\n"
            "             [-l MaxSeedLength] [-e HybridizationEnergyThreshold] [-f InteractionEnergyThreshold]\n"
            "             [-x DropOutLengthInGappedExtension] [-y DropOutLengthInUngappedExtension]\n"
            "             [-g OutputEnergyThreshold] [-s OutputStyle] [-a ParallelAlgorithm] [-p TemporaryPath]\n"
            "\n"
            "  Options:\n"
            "(Required)\n"
            "    -i STR    RNA sequences in FASTA format\n"
            "    -d STR    Input database in pRIblast format\n"
            "    -o STR    Output file name\n"
            "\n"
            "(Optional)\n"
            "    -l INT    Max size of seed length [default:20]\n"
            "    -e DBL    Hybridization energy threshold for seed search [default: -6.0]\n"
            "    -f DBL    Interaction energy threshold for removal of the interaction candidate before gapped "
            "extension [default: -4.0]\n"
            "    -x INT    Dropout Length in gapped extension [default:16]\n"
            "    -y INT    Dropout Length in ungapped extension [default:5]\n"
            "    -g DBL    Energy threshold for output [default:-8.0]\n"
            "    -s INT    Designation of output format style. 0:simplified output, or 1:detailed output [default:0]\n"
            "    -m INT    Minimum helix length in gapped extension [default:3]\n"
            "    -a STR    accepted for compatibility (block, area, dynamic); ignored\n"
            "    -p STR    accepted for compatibility; ignored\n"
            "    -b        write binary hit records instead of text; `pRIblast-hip txt -i FILE -o TEXT` converts\n"
            "    -t        one summary line per query-target pair: hit count, minimum and summed interaction energy,\n"
            "              the best hit's energies and base-pair ends (-s has no effect; not with -b, nor with WORLD_SIZE > 1)\n"
            "    -n INT    with -t: only the INT pairs of lowest minimum interaction energy per query, best first\n"
            "              (ties in -t order; 1 <= INT <= 1024)\n"
            "    -q        one line per query position covered by a final hit: hits and distinct targets covering it,\n"
            "              their minimum interaction energy and its first hit (-s has no effect; not with -t, -n, -b,\n"
            "              nor with WORLD_SIZE > 1)\n"
            "    -k INT    only the INT interaction sites of lowest interaction energy per query, best first, as normal\n"
            "              result lines (-s and -b are honoured; ties in output order; 1 <= INT <= 1024; not with -t, -n, -q,\n"
            "              nor with WORLD_SIZE > 1)\n"
            "    -u        only the distinct interaction sites of each query-target pair: a pair's hits are taken best\n"
            "              first (interaction energy, ties in output order), and a hit is kept only if its query range and\n"
            "              its target range do not both overlap those of a hit kept before it; the lines are lines of the\n"
            "              run without -u (with every other switch; -t, -n, -q and -k then count and rank the kept hits)\n"
            "    -j        only the best co-linear chain of sites of each query-target pair: the hits that follow one\n"
            "              another in the query and in the target without sharing a position of either, chosen for the lowest\n"
            "              summed interaction energy (ties to the earlier hit in output order) - the sites that can bind at\n"
            "              the same time; the lines are lines of the run without -j, and -t's hit count and summed energy are\n"
            "              the chain's (with every switch that -u goes with; not with -u)\n"
            "    -r INT    the -t lines of only the INT queries of lowest minimum interaction energy per target (database\n"
            "              sequence) over all the queries, written at the end of the run by page, target and rank (ties by\n"
            "              the query's place in the input file; 1 <= INT <= 1024; not with -t, -n, -q, -k, -b, nor with\n"
            "              WORLD_SIZE > 1; -u and -j combine)\n"
            "    -c INT    one line per region of a target (database sequence): a maximal run of its positions that final\n"
            "              hits of at least INT distinct queries cover, with the hits that begin in it, the deepest\n"
            "              coverage and where it peaks, the minimum interaction energy and its hit, written at the end of\n"
            "              the run by page, target and start (1 <= INT <= 1000000; not with -t, -n, -q, -k, -b, -r, nor with\n"
            "              WORLD_SIZE > 1; -u and -j combine)\n"
            "    -L STR    search only the query-target pairs listed in the file STR: one pair per line, query name, a tab,\n"
            "              target name, as the result lines print them; `*` as the query name means every query; empty lines\n"
            "              and lines that begin with # are skipped.  The seeds of all other pairs are dropped on the GPU, so\n"
            "              the stages behind cost what the listed pairs cost; the lines are lines of the run without -L (a\n"
            "              query's first line may list its base pairs in another order).  With every other switch\n"
            "    -z INT    with -t: an empirical p-value per query-target pair from INT dinucleotide-preserving shuffles\n"
            "              (decoys) of each query, searched like the query: behind every -t line the decoys per query, how\n"
            "              many of them have a hit against the target (NullHits), how many of those reach the pair's minimum\n"
            "              interaction energy or below (NullLE), the lowest decoy minimum (NullMin, NA without one) and\n"
            "              PValue = (NullLE + 1) / (INT + 1); lines by query, then page, then target (1 <= INT <= 100000;\n"
            "              with -u, -j, -L and the search options; not with -n, -k, -q, -r, -c, -b; PRB_SPLIT has no effect;\n"
            "              PRB_NULL_MASK=0: the decoys are searched against every target, the output is the same)\n"
            "    -Z INT    with -z or -P, with -F, or with -E: the seed of the shuffles [default:1]\n"
            "    -H INT    with -t -z N: sequential p-values (Besag & Clifford 1991).  The decoys 0 .. N - 1 of a query are searched\n"
            "              in rounds of R (-D), and at the end of a round - after R, 2 R, ... and N decoys - a pair that INT or more\n"
            "              of its decoys so far have reached (NullLE >= INT) retires: its p-value is large and known well enough.\n"
            "              It takes no more decoys, and its line is the line of -t -z SEEN, SEEN the decoys it has seen: Decoys =\n"
            "              SEEN, NullHits, NullLE and NullMin over the decoys 0 .. SEEN - 1, PValue = (NullLE + 1) / (SEEN + 1) -\n"
            "              never below Besag & Clifford's INT / SEEN.  Only the pairs that are still candidates for a small p-value\n"
            "              see all N decoys; a query whose pairs have all retired gets no further decoy.  The retiring and the\n"
            "              mask of the live pairs that the next round is searched under are made on the GPU.  The lines and\n"
            "              their order are those of -z; -H N -D N writes the bytes of -t -z N (1 <= INT <= N; not with -P, -F,\n"
            "              -E; the output depends on N, INT, R and -Z only - not on PRB_BATCH, PRB_DEVICES, PRB_SPLIT or\n"
            "              PRB_NULL_MASK=0, which searches every round against every target)\n"
            "    -D INT    with -H: the decoys per round, R; the last round may be short [default:10; 1 <= INT <= N]\n"
            "    -Q        with -t -z N: a Benjamini-Hochberg q-value per query-target pair, ranked on the GPU.  A query is tested\n"
            "              against every target it is searched against - Tests of them: the targets of the database, under -L\n"
            "              the targets listed for the query; a target without a hit has p = 1.  Behind every -z line Tests, Rank =\n"
            "              the query's lines whose PValue is not above the line's (as exact fractions: 1/2 and 2/4 are equal), and\n"
            "              QValue = the lowest Tests * PValue / Rank over the query's lines of this PValue or above, at most 1.\n"
            "              With -H the q-values are over the sequential p-values (Besag-Clifford stopping, then Benjamini-\n"
            "              Hochberg).  The lines and their order are those of the run without -Q (with -H, -D, -Z, -u, -j, -L;\n"
            "              not with -P, -F, -E; the output does not depend on PRB_BATCH, PRB_DEVICES, PRB_SPLIT or PRB_NULL_MASK)\n"
            "    -G STR    with -t: one line per query-group pair, folded on the GPU.  The file STR names the groups (genes, say):\n"
            "              one target per line, target name, a tab, group name; empty lines and lines that begin with # are\n"
            "              skipped; a target the file does not list is a group of its own, named like the target.  Every line\n"
            "              is the -t line of the group's best member (lowest minimum interaction energy; ties: the earlier\n"
            "              target of the database), and behind it the group's name, its members with a hit, its targets and\n"
            "              the members' hits; lines by query, then group in database order; with -n N the N best groups of\n"
            "              each query, by rank (with -n, -u, -j, -L and the search options; not with -z, -k, -q, -r, -c, -b,\n"
            "              nor with WORLD_SIZE > 1; the best queries per group: -R)\n"
            "    -P INT    with -t -G: an empirical p-value per query-group pair from INT shuffled decoys of each query, as -z\n"
            "              makes them: behind every -t -G line the decoys per query, how many of them have a hit against a\n"
            "              target of the group (NullHits), how many of those reach the group's minimum interaction energy or\n"
            "              below on any of its targets - whether or not the query itself hits that target - (NullLE; a decoy\n"
            "              counts once), the lowest decoy minimum (NullMin, NA without one) and PValue = (NullLE + 1) /\n"
            "              (INT + 1); with -n N only the N kept groups of each query get decoys searched against them\n"
            "              (1 <= INT <= 100000; with -n, -u, -j, -L and the search options; not with -z, -k, -q, -r, -c, -b, nor\n"
            "              with WORLD_SIZE > 1; PRB_SPLIT has no effect; PRB_NULL_MASK=0: the decoys are searched against every\n"
            "              target - every listed one under -L -, the output is the same)\n"
            "    -E INT    with -k: an E-value and an FDR q-value per interaction site from INT shuffled decoys of each query, as\n"
            "              -z makes them, searched against the whole database (under -L: against the query's listed targets)\n"
            "              and pooled into one null distribution of hit energies per query: behind every -k line the decoys per\n"
            "              query, the decoy hits at or below the line's interaction energy (NullLE), the query's hits at or\n"
            "              below it (Rank), EValue = NullLE / INT and QValue = the lowest NullLE / (INT * Rank) over the query's\n"
            "              hits of this energy or above, at most 1.  There is no decoy mask: -E INT costs about INT + 1\n"
            "              searches per query, and the pooled null has millions of energies with INT = 5 to 10 - keep INT small\n"
            "              (1 <= INT <= 100000; with -u, -j, -L, -s and the search options; not with -b, -t, -n, -q, -r, -c, -z,\n"
            "              -G, -P, nor with WORLD_SIZE > 1; PRB_SPLIT has no effect)\n"
            "    -R INT    with -t -G: the -t -G lines of only the INT queries of lowest minimum interaction energy per group\n"
            "              over all the queries, written at the end of the run by group in database order, then rank (ties by\n"
            "              the query's place in the input file; 1 <= INT <= 1024; with -u, -j, -L and the search options; not\n"
            "              with -n, -P, nor with what -G can't be combined with; with one process per GPU, WORLD_SIZE > 1,\n"
            "              it is not implemented; the output does not depend on PRB_BATCH, PRB_DEVICES or PRB_SPLIT)\n"
            "    -A STR    with -t: one line per query-feature pair, folded on the GPU.  The file STR annotates the targets: one\n"
            "              feature per line, target name, a tab, start, a tab, end, a tab, feature name; the coordinates are those\n"
            "              the result lines print (0-based, inclusive); empty lines and lines that begin with # are skipped; a\n"
            "              target's features may overlap, nest or repeat, and a target the file does not list has none.  A\n"
            "              final hit belongs to every feature of its target that its span on the target - from the first to\n"
            "              the last base pair - shares a position with.  Every line is the -t line over the feature's hits,\n"
            "              and behind it the feature's name, its start-end and the hits that lie wholly inside it; lines by\n"
            "              query, then target in database order, then the target's features by start, end and line (with\n"
            "              -u, -j, -L and the search options; -s has no effect; not with -n, -z, -k, -q, -r, -c, -b, -G, -P, -E,\n"
            "              -R, nor with WORLD_SIZE > 1; the output does not depend on PRB_BATCH, PRB_DEVICES or PRB_SPLIT;\n"
            "              the best queries per feature: -B)\n"
            "    -F INT    with -t -A: an empirical p-value per query-feature pair from INT shuffled decoys of each query, as -z\n"
            "              makes them: behind every -t -A line the decoys per query, how many of them have a hit whose span\n"
            "              meets the feature (NullHits), how many of those reach the line's minimum interaction energy or below\n"
            "              with such a hit (NullLE; a decoy counts once per feature, and in every feature its hit meets), the\n"
            "              lowest decoy minimum (NullMin, NA without one) and PValue = (NullLE + 1) / (INT + 1); the decoys are\n"
            "              searched against the targets of their query's lines only (1 <= INT <= 100000; with -u, -j, -L, -Z and\n"
            "              the search options; -s has no effect; not with what -A can't be combined with, nor with\n"
            "              WORLD_SIZE > 1; PRB_SPLIT has no effect; the output does not depend on PRB_BATCH or PRB_DEVICES;\n"
            "              PRB_NULL_MASK=0: the decoys are searched against every target - every listed one under -L -, the\n"
            "              output is the same)\n"
            "    -N INT    with -t -A: only the INT lines of lowest minimum interaction energy per query, best first (ties in\n"
            "              -t -A order), chosen on the GPU before the records leave it; the lines are lines of the run without\n"
            "              -N.  With -F the decoys are searched against the targets of each query's INT kept lines only, and\n"
            "              the null columns of a kept line are those of the run without -N (1 <= INT <= 1024; with -F, -u, -j,\n"
            "              -L, -Z and the search options; not with what -A can't be combined with, nor with WORLD_SIZE > 1;\n"
            "              the output does not depend on PRB_BATCH, PRB_DEVICES or PRB_SPLIT)\n"
            "    -B INT    with -t -A: the -t -A lines of only the INT queries of lowest minimum interaction energy per feature\n"
            "              over all the queries, written at the end of the run by feature, then rank (ties by the query's place\n"
            "              in the input file).  The features are numbered in the order of the annotation file's lines; a line\n"
            "              whose target name several database sequences carry is one feature of each, in database order.  A\n"
            "              feature that no query touches writes nothing (1 <= INT <= 1024; with -u, -j, -L and the search\n"
            "              options; -s has no effect; not with -F, -N, nor with what -A can't be combined with; with one process\n"
            "              per GPU, WORLD_SIZE > 1, it is not implemented; the output does not depend on PRB_BATCH,\n"
            "              PRB_DEVICES or PRB_SPLIT)\n"
            "\n"
            "  Environment: PRB_DEVICES=0,1,..  GPUs (workers) of this process;  PRB_BATCH=N  queries per batch [default 2048];\n"
            "               PRB_SPLIT=auto|queries|pages  what the workers share out: whole batches of queries, or the pages of\n"
            "               every batch (a database built with `db -c`); auto [default]: pages when there are fewer batches\n"
            "               than workers; the output is the same; ignored with WORLD_SIZE > 1;\n"
            "               WORLD_SIZE / RANK / LOCAL_RANK  one process per GPU, final hits gathered on rank 0 over RCCL");
}

// An error ends the run: at once - except in a thread of a team (run_team), which hands the message to the main thread
// instead (an exit under the feet of the other workers of a batch would leave their GPUs mid-kernel).
struct TeamError {
  std::string msg;
};
thread_local bool t_team_thread = false;
[[noreturn]] void die(const std::string &msg) {
  if (t_team_thread) throw TeamError{msg};
  std::fprintf(stderr, "%s\n", msg.c_str());
  std::exit(1);
}

// What a run writes, decided once after parsing (output_mode): a line or record per hit, `-t` a line per pair,
// `-t -n` the N best pairs per query, `-q` a line per covered query position, `-k` the N best hits per query, `-r` the
// N best pairs per target, `-c` the regions of each target that enough queries cover, `-t -G` a line per query-group pair,
// `-t -G -P` the same with the group's null columns, `-k -E` the `-k` lines with each hit's score, `-t -G -R` the N best
// query-group pairs per group, `-t -A` a line per query-feature pair, `-t -A -F` the same with the feature's null columns,
// `-t -A -B` the N best query-feature pairs per feature
// (`-N K` chooses no mode of its own: kFeatures and kFeatureNull then finish their table with each query's K best records).
enum class OutputMode { kHits, kSummary, kTop, kProfile, kTopHits, kTargets, kCoverage, kNull, kGroups, kGroupNull, kScored, kGroupRank, kFeatures, kFeatureNull, kFeatureRank };
// -z, -P, -E, -F: a batch is searched with its decoys behind it, into tables that the mode's own function makes and finishes
// (search_null_batch, search_gnull_batch, search_scored_batch, search_fnull_batch) - and by one worker: there is no merge of two of them
constexpr bool runs_decoys(OutputMode m) {
  return m == OutputMode::kNull || m == OutputMode::kGroupNull || m == OutputMode::kScored || m == OutputMode::kFeatureNull;
}

// The switches that choose it, one row each: the description the messages carry, what a switch can't be combined with,
// what it needs, and whether it is refused with one process per GPU (the gather carries hit records only).  The refusals
// are generated from this table (check_switches, check_rank_mode) and keep their precedence: the rows from the last to the
// first, a row's partners from the first to the last.
enum Switch { kT, kN, kQ, kK, kB, kU, kJ, kR, kC, kZ, kZSeed, kG, kP, kE, kGR, kA, kF, kFN, kFB, kH, kHRound, kQValue, kSwitches };
constexpr unsigned bit(Switch s) { return 1u << s; }
struct SwitchRow {
  char letter;
  const char *what;
  unsigned not_with; // bits of Switch
  int needs;         // a Switch, or -1
  bool not_in_rank_mode;
};
constexpr SwitchRow kSwitchTable[kSwitches] = {
    {'t', "per-pair summary lines", bit(kB), -1, true},
    {'n', "the N best pairs per query", 0, kT, false},
    {'q', "per-position profile lines", bit(kT) | bit(kN) | bit(kB), -1, true},
    {'k', "the N best interaction sites per query", bit(kT) | bit(kN) | bit(kQ), -1, true},
    {'b', "binary hit records", 0, -1, false},
    {'u', "the distinct interaction sites of each pair", 0, -1, false},
    {'j', "the best co-linear chain of sites of each pair", bit(kU), -1, false},
    {'r', "the N best queries per target", bit(kT) | bit(kN) | bit(kQ) | bit(kK) | bit(kB), -1, true},
    {'c', "the regions of each target bound by at least D queries", bit(kT) | bit(kN) | bit(kQ) | bit(kK) | bit(kB) | bit(kR), -1, true},
    {'z', "an empirical p-value per pair from N shuffled decoys", bit(kN) | bit(kK) | bit(kQ) | bit(kR) | bit(kC) | bit(kB), kT, true},
    {'Z', "the seed of the decoys' shuffles", 0, kZ, false},
    {'G', "one line per query-group pair", bit(kZ) | bit(kK) | bit(kQ) | bit(kR) | bit(kC) | bit(kB), kT, true},
    {'P', "an empirical p-value per query-group pair from N shuffled decoys", bit(kZ) | bit(kK) | bit(kQ) | bit(kR) | bit(kC) | bit(kB), kG, true},
    {'E', "an E-value and a q-value per interaction site from N pooled decoys per query",
     bit(kB) | bit(kT) | bit(kN) | bit(kQ) | bit(kR) | bit(kC) | bit(kZ) | bit(kG) | bit(kP), kK, true},
    // (what -G can't be combined with, and one process per GPU, are refused through -G's row, in its words)
    {'R', "the N best queries per group", bit(kN) | bit(kP), kG, false},
    {'A', "one line per query-feature pair",
     bit(kN) | bit(kQ) | bit(kK) | bit(kB) | bit(kR) | bit(kC) | bit(kZ) | bit(kG) | bit(kP) | bit(kE) | bit(kGR), kT, true},
    {'F', "an empirical p-value per query-feature pair from N shuffled decoys",
     bit(kN) | bit(kQ) | bit(kK) | bit(kB) | bit(kR) | bit(kC) | bit(kZ) | bit(kG) | bit(kP) | bit(kE) | bit(kGR), kA, true},
    // (what -A can't be combined with, and one process per GPU, are refused through -A's row, in its words)
    {'N', "the N best features per query", 0, kA, false},
    // (likewise)
    {'B', "the N best queries per feature", bit(kF) | bit(kFN), kA, false},
    // (-P, -F and -E make decoys of their own and are refused with -z: -H is refused with them through its need of -z)
    {'H', "sequential p-values: a pair takes no more decoys once H of them reach its minimum energy", 0, kZ, false},
    {'D', "the decoys per round of the sequential p-values", 0, kH, false},
    // (likewise: -P, -F and -E are refused with -Q through its need of -z)
    {'Q', "a Benjamini-Hochberg q-value per pair of the null table", 0, kZ, false},
};
std::string described(int s) { return std::string("-") + kSwitchTable[s].letter + " (" + kSwitchTable[s].what + ")"; }

struct Args {
  std::string in, out, db, tmp;
  std::string pairlist; // -L
  bool have_pairlist = false;
  std::string groupfile; // -G
  std::string annotfile; // -A
  prb_ris_opts o;
  bool given[kSwitches] = {};
  int top = 0, tophits = 0, targets = 0, depth = 0; // the values of -n, -k, -r and -c (-1: not a count)
  int grouprank = 0;                                // -R, likewise
  int feattop = 0;                                  // -N, likewise
  int featrank = 0;                                 // -B, likewise
  int decoys = 0;                                   // -z, -P, -E or -F, likewise
  int retire_le = 0, round = 10;                    // -H and -D, likewise
  uint64_t shuffle_seed = 1;                        // -Z
  bool seed_ok = true;                              // -Z's value is a non-negative integer
  OutputMode mode = OutputMode::kHits;
  bool binary() const { return given[kB]; }
};

struct Worker {
  int device;
  prb_ctx *ctx = nullptr, *prep_ctx = nullptr; // prep_ctx: accessibilities of the next batch, on a stream of its own
  prb_db *db = nullptr;
  prb_targetset *targets = nullptr;                   // -r: this worker's table, for the whole run
  prb_covset *coverage = nullptr;                     // -c: this worker's table, for the whole run
  prb_grouprank *grouprank = nullptr;                 // -R: this worker's table, for the whole run
  prb_annot *annot = nullptr;                         // -A: the annotation on this worker's device, for the whole run
  prb_featrank *featrank = nullptr;                   // -B: this worker's table, for the whole run
  std::vector<std::pair<int32_t, int32_t>> target_qlen; // -r, -c, -R, -B: (input position, unmasked length) of the queries it prepared
};

// The one place where what a search returned is freed.
struct Free {
  void operator()(prb_hitset *p) const { prb_hitset_free(p); }
  void operator()(prb_pairset *p) const { prb_pairset_free(p); }
  void operator()(prb_topset *p) const { prb_topset_free(p); }
  void operator()(prb_profset *p) const { prb_profset_free(p); }
  void operator()(prb_tophits *p) const { prb_tophits_free(p); }
  void operator()(prb_nullset *p) const { prb_nullset_free(p); }
  void operator()(prb_groupset *p) const { prb_groupset_free(p); }
  void operator()(prb_gnullset *p) const { prb_gnullset_free(p); }
  void operator()(prb_featset *p) const { prb_featset_free(p); }
  void operator()(prb_fnullset *p) const { prb_fnullset_free(p); }
  void operator()(prb_evalset *p) const { prb_evalset_free(p); }
  void operator()(prb_qbatch *p) const { prb_qbatch_destroy(p); }
  void operator()(prb_pairmask *p) const { prb_pairmask_free(p); }
};
template <class T> using Handle = std::unique_ptr<T, Free>;

// What a searched batch left, by mode: hit sets or pair sets (one per database page), or the one table that every page
// was merged into on the device.
struct BatchResult {
  OutputMode mode = OutputMode::kHits;
  std::vector<Handle<prb_hitset>> pages;       // kHits
  std::vector<Handle<prb_pairset>> pair_pages; // kSummary
  Handle<prb_topset> top;                      // kTop
  Handle<prb_profset> prof;                    // kProfile
  Handle<prb_tophits> tophits;                 // kTopHits
  Handle<prb_nullset> null;                    // kNull
  Handle<prb_groupset> groups;                 // kGroups; kGroupRank: until it is merged into the worker's table
  Handle<prb_gnullset> gnull;                  // kGroupNull
  Handle<prb_featset> features;                // kFeatures; kFeatureRank: until it is merged into the worker's table
  Handle<prb_fnullset> fnull;                  // kFeatureNull
  std::vector<prb_eval_score> scores;          // kScored: of the records of `tophits`, in their order
};

// The result of one batch (in rank mode: of one round of batches, gathered), waiting to be written.
struct BatchJob {
  BatchResult res;
  std::vector<std::string> names; // of its queries, in the order of their indices in the hit records
  std::vector<int32_t> qlen_unmasked;
};

// A batch with its accessibilities computed, ready to be searched.
struct Prepared {
  prb_qbatch *qb = nullptr;
  prb_pairmask *mask = nullptr; // -L: the listed pairs of its queries
  std::vector<int32_t> qlen_unmasked;
  std::vector<int32_t> ids; // its queries' positions in the input file (-r: their identifiers in the table)
};

// ---- binary hit file (little-endian, the layouts of include/priblast_hip.h) ----------------------
//   "PRBHITS\1" | i32 output_style | i32 npages | str header (the three text lines)
//   per page: i32 nseq, then per sequence i32 length, i32 length_unmasked, i32 start_pos, str name
//   blocks:   i64 'B' | i64 nq | per query: str name, i32 length_unmasked
//             | per page: i64 nhits, i64 npairs, prb_hit[nhits], int32[2 * npairs]
//   trailer:  i64 'E' | i64 total hits
//   str = i32 length + bytes.  prb_hit.bp_offset indexes the pair array of its own block and page.
constexpr char kMagic[8] = {'P', 'R', 'B', 'H', 'I', 'T', 'S', 1};
constexpr int64_t kBlock = 'B', kEnd = 'E';

void put(std::FILE *f, const void *p, size_t n) {
  if (n && std::fwrite(p, 1, n, f) != n) die("Error: can't write the output file");
}
template <class T> void put(std::FILE *f, T v) { put(f, &v, sizeof v); }
void put_str(std::FILE *f, const std::string &s) {
  put<int32_t>(f, (int32_t)s.size());
  put(f, s.data(), s.size());
}
void get(std::FILE *f, void *p, size_t n) {
  if (n && std::fread(p, 1, n, f) != n) die("Error: truncated binary hit file");
}
template <class T> T get(std::FILE *f) {
  T v;
  get(f, &v, sizeof v);
  return v;
}
std::string get_str(std::FILE *f) {
  const int32_t n = get<int32_t>(f);
  if (n < 0 || n > (1 << 28)) die("Error: corrupt binary hit file");
  std::string s((size_t)n, '\0');
  get(f, s.data(), s.size());
  return s;
}

void write_binary_head(std::FILE *f, int output_style, const std::string &header, const std::vector<SeqTable> &tabs) {
  put(f, kMagic, sizeof kMagic);
  put<int32_t>(f, output_style);
  put<int32_t>(f, (int32_t)tabs.size());
  put_str(f, header);
  for (const SeqTable &t : tabs) {
    put<int32_t>(f, (int32_t)t.names.size());
    for (size_t i = 0; i < t.names.size(); i++) {
      put<int32_t>(f, t.len[i]);
      put<int32_t>(f, t.len_unmasked[i]);
      put<int32_t>(f, t.start_pos[i]);
      put_str(f, t.names[i]);
    }
  }
}

int64_t write_binary_batch(const BatchView &v, std::FILE *f) {
  put<int64_t>(f, kBlock);
  put<int64_t>(f, (int64_t)v.nq);
  for (size_t q = 0; q < v.nq; q++) {
    put_str(f, v.names[q]);
    put<int32_t>(f, v.qlen_unmasked[q]);
  }
  int64_t total = 0;
  for (const PageHits &p : v.pages) {
    put<int64_t>(f, p.n);
    put<int64_t>(f, p.nbp);
    put(f, p.h, (size_t)p.n * sizeof(prb_hit));
    put(f, p.bp, (size_t)p.nbp * 2 * sizeof(int32_t));
    total += p.n;
  }
  return total;
}

// `txt` sub-command: binary hit file -> the text `ris` writes.
int txt_main(int argc, char **argv) {
  std::string in, out;
  int c;
  while ((c = getopt(argc, argv, "i:o:")) != -1) {
    switch (c) {
    case 'i': in = optarg; break;
    case 'o': out = optarg; break;
    default: die("Error: invalid argument");
    }
  }
  std::FILE *f = std::fopen(in.c_str(), "rb");
  if (!f) die("Error: can't open input_file: " + in);
  char magic[8];
  get(f, magic, sizeof magic);
  if (std::memcmp(magic, kMagic, sizeof kMagic)) die("Error: " + in + " is not a binary hit file");
  const int output_style = get<int32_t>(f);
  const int np = get<int32_t>(f);
  if (np < 0 || np > (1 << 24)) die("Error: corrupt binary hit file");
  const std::string header = get_str(f);
  std::vector<SeqTable> tabs((size_t)np);
  for (SeqTable &t : tabs) {
    const int32_t nseq = get<int32_t>(f);
    if (nseq < 0) die("Error: corrupt binary hit file");
    for (int32_t i = 0; i < nseq; i++) {
      t.len.push_back(get<int32_t>(f));
      t.len_unmasked.push_back(get<int32_t>(f));
      t.start_pos.push_back(get<int32_t>(f));
      t.names.push_back(get_str(f));
    }
  }
  std::FILE *o = std::fopen(out.c_str(), "w");
  if (!o) die("Error: can't open output_file: " + out);
  put(o, header.data(), header.size());
  if (std::fflush(o)) die("Error: can't write the output file");
  LineSink sink;
  sink.fd = fileno(o);
  int64_t id = 0;
  for (;;) {
    const int64_t tag = get<int64_t>(f);
    if (tag == kEnd) {
      if (get<int64_t>(f) != id) die("Error: corrupt binary hit file (hit count)");
      break;
    }
    if (tag != kBlock) die("Error: corrupt binary hit file");
    const int64_t nq = get<int64_t>(f);
    if (nq < 0 || nq > (1 << 28)) die("Error: corrupt binary hit file");
    std::vector<std::string> names((size_t)nq);
    std::vector<int32_t> qlen((size_t)nq);
    for (int64_t q = 0; q < nq; q++) {
      names[q] = get_str(f);
      qlen[q] = get<int32_t>(f);
    }
    std::vector<std::vector<prb_hit>> hits((size_t)np);
    std::vector<std::vector<int32_t>> pairs((size_t)np);
    BatchView v;
    v.nq = (size_t)nq;
    v.names = names.data();
    v.qlen_unmasked = qlen.data();
    for (int p = 0; p < np; p++) {
      const int64_t n = get<int64_t>(f), nbp = get<int64_t>(f);
      if (n < 0 || nbp < 0) die("Error: corrupt binary hit file");
      hits[p].resize((size_t)n);
      pairs[p].resize((size_t)nbp * 2);
      get(f, hits[p].data(), (size_t)n * sizeof(prb_hit));
      get(f, pairs[p].data(), (size_t)nbp * 2 * sizeof(int32_t));
      for (const prb_hit &x : hits[p])
        if (x.query < 0 || x.query >= nq || x.db_id < 0 || (size_t)x.db_id >= tabs[p].names.size() || x.bp_count < 0 ||
            x.bp_offset < 0 || x.bp_offset + x.bp_count > nbp)
          die("Error: corrupt binary hit file (record)");
      PageHits ph;
      ph.h = hits[p].data();
      ph.n = n;
      ph.bp = pairs[p].data();
      ph.nbp = nbp;
      v.pages.push_back(ph);
    }
    id = prb::format_batch(v, tabs, output_style, id, sink, prb::format_threads());
    if (id < 0) die("Error: can't write the output file");
  }
  std::fclose(f);
  if (std::fclose(o)) die("Error: can't write the output file");
  return 0;
}

// The RCCL id of a multi-process run travels through files in the `-p` directory.  A file left behind by a run that
// died must never be taken for this run's (ncclCommInitRank would wait for ever on a stale id), and file times say
// nothing reliable about that, so the exchange is a handshake: every other rank writes a random nonce to
// `<path>.hello.<rank>`; rank 0 publishes `<path>` = the id followed by the nonces it has seen, and publishes again
// whenever a hello file changes (a stale hello of a dead run is simply overwritten by the live rank); a rank takes
// the id only from a file that carries ITS nonce.  Rank 0 keeps publishing until its communicator exists - which is
// when every rank has the id - and then removes the files.  A rank that fails kills the job under torchrun / mpirun;
// started by hand, the others give up after PRB_RENDEZVOUS_TIMEOUT seconds (default 300) instead of waiting for it.
struct Rendezvous {
  std::string path;
  int world = 1, rank = 0;
  char id[PRB_COMM_ID_BYTES] = {};
  std::thread publisher;
  std::atomic<bool> stop{false};

  static uint64_t nonce() {
    uint64_t v = 0;
    if (std::FILE *f = std::fopen("/dev/urandom", "rb")) {
      if (std::fread(&v, sizeof v, 1, f) != 1) v = 0;
      std::fclose(f);
    }
    return v ? v : ((uint64_t)getpid() << 32) ^ (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
  }
  static bool write_atomic(const std::string &p, const void *data, size_t n) {
    const std::string tmp = p + ".tmp";
    std::FILE *f = std::fopen(tmp.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(data, 1, n, f) == n;
    return (std::fclose(f) == 0) && ok && std::rename(tmp.c_str(), p.c_str()) == 0;
  }
  static bool read_exact(const std::string &p, void *data, size_t n) {
    struct stat st;
    if (stat(p.c_str(), &st) != 0 || (size_t)st.st_size != n) return false;
    std::FILE *f = std::fopen(p.c_str(), "rb");
    if (!f) return false;
    const bool ok = std::fread(data, 1, n, f) == n;
    std::fclose(f);
    return ok;
  }
  static int timeout_s() {
    const char *e = std::getenv("PRB_RENDEZVOUS_TIMEOUT");
    return e ? std::max(1, std::atoi(e)) : 300;
  }
  std::string hello(int r) const { return path + ".hello." + std::to_string(r); }

  void begin(const std::string &p, int world_, int rank_) {
    path = p;
    world = world_;
    rank = rank_;
    const size_t full = PRB_COMM_ID_BYTES + 8 * (size_t)(world - 1);
    if (rank == 0) {
      std::remove(path.c_str());
      std::remove((path + ".tmp").c_str());
      if (prb_comm_unique_id(id)) die(std::string("Error: ") + prb_last_error());
      if (world == 1) return;
      publisher = std::thread([this, full] {
        std::vector<uint64_t> seen((size_t)(world - 1), 0), now((size_t)(world - 1), 0);
        std::vector<char> buf(full);
        while (!stop.load()) {
          bool all = true;
          for (int r = 1; r < world; r++) all = read_exact(hello(r), &now[(size_t)r - 1], 8) && now[(size_t)r - 1] != 0 && all;
          if (all && now != seen) {
            std::memcpy(buf.data(), id, PRB_COMM_ID_BYTES);
            std::memcpy(buf.data() + PRB_COMM_ID_BYTES, now.data(), 8 * now.size());
            if (!write_atomic(path, buf.data(), full)) die("Error: can't write the rendezvous file " + path);
            seen = now;
          }
          std::this_thread::sleep_for(std::chrono::milliseconds(10));
        }
      });
      return;
    }
    const uint64_t mine = nonce();
    if (!write_atomic(hello(rank), &mine, 8)) die("Error: can't write the rendezvous file " + hello(rank));
    std::vector<char> buf(full);
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      uint64_t got = 0;
      if (read_exact(path, buf.data(), full)) std::memcpy(&got, buf.data() + PRB_COMM_ID_BYTES + 8 * (size_t)(rank - 1), 8);
      if (got == mine) break;
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(timeout_s()))
        die("Error: no rendezvous file " + path + " from rank 0 (is it running? a rank that fails must end the whole job)");
      std::this_thread::sleep_for(std::chrono::milliseconds(10));
    }
    std::memcpy(id, buf.data(), PRB_COMM_ID_BYTES);
  }
  // after prb_comm_create returned on this rank (on rank 0: every rank has joined the communicator, so has the id)
  void end() {
    if (rank != 0) return;
    stop.store(true);
    if (publisher.joinable()) publisher.join();
    std::remove(path.c_str());
    for (int r = 1; r < world; r++) std::remove(hello(r).c_str());
  }
};

// ---- the run: what the steps of ris_main fill in, one after the other, and the workers read --------
// -L: the listed pairs, by the query's place in the input file (`of_query`) and for every query (`every`: the `*`
// lines), as targets numbered page by page; page_first[p] = the first target of page p
struct PairList {
  std::vector<std::vector<int64_t>> of_query;
  std::vector<int64_t> every;
  std::vector<int64_t> page_first; // [npages + 1]
};

// -G: the group of every database sequence, per page; the groups numbered by their first member in database order
struct GroupMap {
  std::vector<std::vector<int32_t>> of_page;
  std::vector<std::string> names;
  std::vector<int32_t> sizes; // targets per group
  std::vector<std::vector<std::pair<int32_t, int32_t>>> members; // -P: per group its targets (page, db_id), in database order
};

// -A: the features of the database's sequences in the file's order, as prb_annot_create takes them, and their names
struct Annotation {
  std::vector<int32_t> page, db_id, start, end;
  std::vector<std::string> names;
};

struct Run {
  Args a;
  PairList list;
  GroupMap groups;
  Annotation annot;
  std::vector<std::string> names, seqs; // the queries
  int world = 1, rank = 0;              // one process per GPU?  (torchrun / mpirun style environment)
  bool rank_mode = false;
  prb_comm *comm = nullptr;
  std::vector<Worker> workers;
  int repeat_flag = 0, W = 0, delta = 0, npages = 0; // of the database
  std::vector<SeqTable> tabs;                        // per page
  std::FILE *out = nullptr;
  // the batch plan: batch b = the queries order[b * batch ..), nb batches, njobs jobs for the writer
  std::vector<size_t> order;
  size_t batch = 1, nb = 0, njobs = 0;
  // PRB_SPLIT: what the workers of one process share out (plan_split)
  int split_knob = 0;       // index in kSplitNames
  bool split_given = false; // PRB_SPLIT is set
  bool split_pages = false; // this run: the pages of every batch
  std::vector<size_t> batch_idx(size_t b) const {
    return std::vector<size_t>(order.begin() + b * batch, order.begin() + std::min(seqs.size(), (b + 1) * batch));
  }
  void names_of(size_t b, std::vector<std::string> &dst) const {
    for (size_t i : batch_idx(b)) dst.push_back(names[i]);
  }
};

// the value of -n / -k / -r / -c: a count, or -1
int parse_count(const char *arg) {
  char *end = nullptr;
  const long v = std::strtol(arg, &end, 10);
  return end != arg && *end == '\0' && v >= 0 && v <= 1 << 20 ? (int)v : -1;
}

// the refusals that need the command line only, from the switch table
void check_switches(const Args &a) {
  for (int s = kSwitches - 1; s >= 0; s--) {
    if (!a.given[s]) continue;
    for (int p = 0; p < kSwitches; p++)
      if (a.given[p] && (kSwitchTable[s].not_with & (1u << p))) die("Error: " + described(s) + " can't be combined with " + described(p));
    // (-Z goes with either switch that makes decoys)
    if (const int need = kSwitchTable[s].needs; need >= 0 && !a.given[need] && !(s == kZSeed && (a.given[kP] || a.given[kE] || a.given[kF]))) die("Error: " + described(s) + " needs " + described(need));
  }
  for (Switch s : {kR, kK, kN, kGR, kFN, kFB})
    if (const int v = s == kR ? a.targets : s == kK ? a.tophits : s == kGR ? a.grouprank : s == kFN ? a.feattop : s == kFB ? a.featrank : a.top; a.given[s] && (v < 1 || v > 1024))
      die(std::string("Error: -") + kSwitchTable[s].letter + " needs an integer between 1 and 1024 (this build's limit)");
  if (a.given[kC] && (a.depth < 1 || a.depth > 1000000)) die("Error: -c needs an integer between 1 and 1000000 (this build's limit)");
  if (a.given[kZ] && (a.decoys < 1 || a.decoys > 100000)) die("Error: -z needs an integer between 1 and 100000 (this build's limit)");
  if (a.given[kP] && (a.decoys < 1 || a.decoys > 100000)) die("Error: -P needs an integer between 1 and 100000 (this build's limit)");
  if (a.given[kE] && (a.decoys < 1 || a.decoys > 100000)) die("Error: -E needs an integer between 1 and 100000 (this build's limit)");
  if (a.given[kF] && (a.decoys < 1 || a.decoys > 100000)) die("Error: -F needs an integer between 1 and 100000 (this build's limit)");
  if (a.given[kZSeed] && !a.seed_ok) die("Error: -Z needs a non-negative integer");
  for (Switch s : {kH, kHRound})
    if (const int v = s == kH ? a.retire_le : a.round; a.given[s] && (v < 1 || v > a.decoys))
      die(std::string("Error: -") + kSwitchTable[s].letter + " needs an integer between 1 and the decoys per query (-z " + std::to_string(a.decoys) + ")");
}

OutputMode output_mode(const Args &a) {
  if (a.given[kE]) return OutputMode::kScored;
  if (a.given[kZ]) return OutputMode::kNull;
  if (a.given[kP]) return OutputMode::kGroupNull;
  if (a.given[kGR]) return OutputMode::kGroupRank;
  if (a.given[kFB]) return OutputMode::kFeatureRank;
  if (a.given[kF]) return OutputMode::kFeatureNull;
  if (a.given[kA]) return OutputMode::kFeatures;
  if (a.given[kG]) return OutputMode::kGroups;
  return a.given[kC] ? OutputMode::kCoverage : a.given[kR] ? OutputMode::kTargets : a.given[kK] ? OutputMode::kTopHits : a.given[kQ] ? OutputMode::kProfile : a.given[kN] ? OutputMode::kTop
         : a.given[kT] ? OutputMode::kSummary : OutputMode::kHits;
}

Args parse_args(int argc, char **argv) {
  Args a;
  prb_ris_opts_default(&a.o);
  int c;
  while ((c = getopt(argc, argv, "i:o:d:l:e:y:x:f:g:s:m:p:a:btn:qk:ujr:c:L:z:Z:G:P:E:R:A:F:N:B:H:D:Q")) != -1) {
    switch (c) {
    case 'i': a.in = optarg; break;
    case 'o': a.out = optarg; break;
    case 'd': a.db = optarg; break;
    case 'l': a.o.max_seed_length = std::atoi(optarg); break;
    case 'e': a.o.hybrid_threshold = std::atof(optarg); break;
    case 'f': a.o.interaction_threshold = std::atof(optarg); break;
    case 'g': a.o.final_threshold = std::atof(optarg); break;
    case 's': a.o.output_style = std::atoi(optarg); break;
    case 'x': a.o.drop_out_w_gap = std::atoi(optarg); break;
    case 'y': a.o.drop_out_wo_gap = std::atoi(optarg); break;
    case 'm': a.o.min_helix_length = std::atoi(optarg); break;
    case 'p': a.tmp = optarg; break;
    case 'b': a.given[kB] = true; break;
    case 't': a.given[kT] = true; break;
    case 'q': a.given[kQ] = true; break;
    case 'u': a.given[kU] = true, a.o.distinct_sites = 1; break;
    case 'j': a.given[kJ] = true, a.o.chain_sites = 1; break;
    case 'n': a.given[kN] = true, a.top = parse_count(optarg); break;
    case 'k': a.given[kK] = true, a.tophits = parse_count(optarg); break;
    case 'r': a.given[kR] = true, a.targets = parse_count(optarg); break;
    case 'c': a.given[kC] = true, a.depth = parse_count(optarg); break;
    case 'L': a.have_pairlist = true, a.pairlist = optarg; break;
    case 'z': a.given[kZ] = true, a.decoys = parse_count(optarg); break;
    case 'G': a.given[kG] = true, a.groupfile = optarg; break;
    case 'A': a.given[kA] = true, a.annotfile = optarg; break;
    case 'P': a.given[kP] = true, a.decoys = parse_count(optarg); break;
    case 'E': a.given[kE] = true, a.decoys = parse_count(optarg); break;
    case 'F': a.given[kF] = true, a.decoys = parse_count(optarg); break;
    case 'R': a.given[kGR] = true, a.grouprank = parse_count(optarg); break;
    case 'N': a.given[kFN] = true, a.feattop = parse_count(optarg); break;
    case 'B': a.given[kFB] = true, a.featrank = parse_count(optarg); break;
    case 'H': a.given[kH] = true, a.retire_le = parse_count(optarg); break;
    case 'D': a.given[kHRound] = true, a.round = parse_count(optarg); break;
    case 'Q': a.given[kQValue] = true; break;
    case 'Z': {
      char *end = nullptr;
      errno = 0;
      a.given[kZSeed] = true;
      a.shuffle_seed = std::strtoull(optarg, &end, 10);
      a.seed_ok = end != optarg && *end == '\0' && errno == 0 && optarg[0] != '-';
      break;
    }
    case 'a':
      if (std::strcmp(optarg, "block") && std::strcmp(optarg, "area") && std::strcmp(optarg, "dynamic"))
        die("Error: parallel algorithm not supported.");
      break;
    default: die("Error: invalid argument");
    }
  }
  check_switches(a);
  a.mode = output_mode(a);
  return a;
}

// the text of the file `path` that a switch names (`what`: "the pair list (-L)")
std::string read_list_file(const std::string &path, const char *what) {
  std::FILE *f = std::fopen(path.c_str(), "r");
  if (!f) die(std::string("Error: can't open ") + what + ": " + path);
  std::string text;
  char buf[1 << 16];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
  const bool bad = std::ferror(f) != 0;
  std::fclose(f);
  if (bad) die(std::string("Error: can't read ") + what + ": " + path);
  return text;
}

// -L FILE: every line checked and turned into targets per query; any fault ends the run here, before any GPU work
void load_pairlist(Run &r) {
  if (!r.a.have_pairlist) return;
  const std::string text = read_list_file(r.a.pairlist, "the pair list (-L)");
  std::vector<std::vector<std::string>> pages;
  if (const std::string err = prb::read_db_names(r.a.db, pages); !err.empty()) die(err); // (no GPU is needed to refuse a list)
  PairList &pl = r.list;
  std::multimap<std::string, int64_t> target_of, query_of; // a name that occurs several times matches all of them
  pl.page_first.assign(1, 0);
  for (const auto &pg : pages) {
    for (const std::string &n : pg) target_of.emplace(n, pl.page_first.back() + (int64_t)(&n - pg.data()));
    pl.page_first.push_back(pl.page_first.back() + (int64_t)pg.size());
  }
  for (size_t q = 0; q < r.names.size(); q++) query_of.emplace(r.names[q], (int64_t)q);
  pl.of_query.resize(r.names.size());
  int64_t allowed = 0;
  size_t lineno = 0;
  for (size_t at = 0; at < text.size();) {
    size_t end = text.find('\n', at);
    if (end == std::string::npos) end = text.size();
    std::string line = text.substr(at, end - at);
    at = end + 1;
    lineno++;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    const size_t tab = line.find('\t');
    if (tab == std::string::npos || line.find('\t', tab + 1) != std::string::npos)
      die("Error: pair list line " + std::to_string(lineno) + ": expected query name, one tab, target name");
    const std::string qn = line.substr(0, tab), tn = line.substr(tab + 1);
    const auto tr = target_of.equal_range(tn);
    if (qn != "*" && query_of.find(qn) == query_of.end()) die("Error: pair list line " + std::to_string(lineno) + ": no query is named \"" + qn + "\"");
    if (tr.first == tr.second) die("Error: pair list line " + std::to_string(lineno) + ": no database sequence is named \"" + tn + "\"");
    for (auto t = tr.first; t != tr.second; ++t) {
      if (qn == "*") {
        pl.every.push_back(t->second);
      } else {
        const auto qr = query_of.equal_range(qn);
        for (auto q = qr.first; q != qr.second; ++q) pl.of_query[(size_t)q->second].push_back(t->second);
      }
      allowed++;
    }
  }
  if (allowed == 0) die("Error: the pair list (-L) allows no pair: " + r.a.pairlist);
}

// -G FILE: every line checked, then every database sequence given its group; any fault ends the run here, before any GPU
// work.  Groups are identified by name; a sequence that the file does not list is in the group named by its own name.
void load_groups(Run &r) {
  if (!r.a.given[kG]) return;
  const std::string text = read_list_file(r.a.groupfile, "the group file (-G)");
  std::vector<std::vector<std::string>> pages;
  if (const std::string err = prb::read_db_names(r.a.db, pages); !err.empty()) die(err); // (no GPU is needed to refuse a file)
  std::map<std::string, bool> in_db;
  for (const auto &pg : pages)
    for (const std::string &n : pg) in_db[n] = true;
  std::map<std::string, std::string> group_of_target;
  size_t lineno = 0;
  for (size_t at = 0; at < text.size();) {
    size_t end = text.find('\n', at);
    if (end == std::string::npos) end = text.size();
    std::string line = text.substr(at, end - at);
    at = end + 1;
    lineno++;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    const std::string where = "Error: group file line " + std::to_string(lineno) + ": ";
    const size_t tab = line.find('\t');
    if (tab == std::string::npos || line.find('\t', tab + 1) != std::string::npos) die(where + "expected target name, one tab, group name");
    const std::string tn = line.substr(0, tab), gn = line.substr(tab + 1);
    if (gn.empty()) die(where + "the group name is empty");
    if (!in_db.count(tn)) die(where + "no database sequence is named \"" + tn + "\"");
    const auto ins = group_of_target.emplace(tn, gn);
    if (!ins.second && ins.first->second != gn)
      die(where + "\"" + tn + "\" is listed with the groups \"" + ins.first->second + "\" and \"" + gn + "\"");
  }
  GroupMap &gm = r.groups;
  std::map<std::string, int32_t> index_of; // groups numbered by their first member in database order
  gm.of_page.resize(pages.size());
  for (size_t p = 0; p < pages.size(); p++)
    for (const std::string &n : pages[p]) {
      const auto listed = group_of_target.find(n);
      const std::string &gn = listed == group_of_target.end() ? n : listed->second;
      const auto ins = index_of.emplace(gn, (int32_t)gm.names.size());
      if (ins.second) {
        gm.names.push_back(gn);
        gm.sizes.push_back(0);
      }
      gm.of_page[p].push_back(ins.first->second);
      gm.sizes[(size_t)ins.first->second]++;
    }
  if (!r.a.given[kP]) return;
  gm.members.resize(gm.names.size());
  for (size_t p = 0; p < gm.of_page.size(); p++)
    for (size_t i = 0; i < gm.of_page[p].size(); i++) gm.members[(size_t)gm.of_page[p][i]].emplace_back((int32_t)p, (int32_t)i);
}

// -A FILE: every line checked and turned into a feature of every database sequence of that name; any fault ends the run
// here, before any GPU work, with the file's name and the line's number.  A sequence that the file does not list has no feature.
void load_features(Run &r) {
  if (!r.a.given[kA]) return;
  const std::string text = read_list_file(r.a.annotfile, "the annotation file (-A)");
  std::vector<std::vector<std::string>> pages;
  std::vector<std::vector<int32_t>> lengths;
  if (const std::string err = prb::read_db_names(r.a.db, pages, &lengths); !err.empty()) die(err); // (no GPU is needed to refuse a file)
  std::multimap<std::string, std::pair<int32_t, int32_t>> target_of; // a name that occurs several times matches all of them
  for (size_t p = 0; p < pages.size(); p++)
    for (size_t i = 0; i < pages[p].size(); i++) target_of.emplace(pages[p][i], std::make_pair((int32_t)p, (int32_t)i));
  Annotation &an = r.annot;
  // a coordinate: digits only, within int32
  auto coordinate = [](const std::string &f, int64_t *v) {
    if (f.empty() || f.size() > 10) return false;
    *v = 0;
    for (char ch : f) {
      if (ch < '0' || ch > '9') return false;
      *v = *v * 10 + (ch - '0');
    }
    return *v <= INT32_MAX;
  };
  size_t lineno = 0;
  for (size_t at = 0; at < text.size();) {
    size_t end = text.find('\n', at);
    if (end == std::string::npos) end = text.size();
    std::string line = text.substr(at, end - at);
    at = end + 1;
    lineno++;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    const std::string where = "Error: annotation file " + r.a.annotfile + " line " + std::to_string(lineno) + ": ";
    std::vector<std::string> f;
    for (size_t a0 = 0;;) {
      const size_t tab = line.find('\t', a0);
      f.push_back(line.substr(a0, tab == std::string::npos ? std::string::npos : tab - a0));
      if (tab == std::string::npos) break;
      a0 = tab + 1;
    }
    int64_t s = 0, e = 0;
    if (f.size() != 4 || f[0].empty() || f[3].empty() || !coordinate(f[1], &s) || !coordinate(f[2], &e))
      die(where + "expected target name, start, end and feature name, separated by tabs (0-based, inclusive coordinates)");
    const auto tr = target_of.equal_range(f[0]);
    if (tr.first == tr.second) die(where + "no database sequence is named \"" + f[0] + "\"");
    if (s > e) die(where + "start " + std::to_string(s) + " is behind end " + std::to_string(e));
    for (auto t = tr.first; t != tr.second; ++t) {
      const int32_t len = lengths[(size_t)t->second.first][(size_t)t->second.second];
      if (e >= len) die(where + "end " + std::to_string(e) + " is outside \"" + f[0] + "\" (length " + std::to_string(len) + ")");
      an.page.push_back(t->second.first);
      an.db_id.push_back(t->second.second);
      an.start.push_back((int32_t)s);
      an.end.push_back((int32_t)e);
      an.names.push_back(f[3]);
    }
  }
  if (r.a.given[kFB] && an.names.empty()) die("Error: annotation file " + r.a.annotfile + " has no feature: " + described(kFB) + " needs one");
}

// -L: the mask of a prepared batch's queries (input positions `ids`)
prb_pairmask *batch_mask(const Run &r, prb_ctx *c, const prb_qbatch *qb, const prb_db *db, const std::vector<int32_t> &ids) {
  const PairList &pl = r.list;
  std::vector<int32_t> query, page, db_id;
  auto add = [&](int32_t q, int64_t t) {
    const size_t p = (size_t)(std::upper_bound(pl.page_first.begin(), pl.page_first.end(), t) - pl.page_first.begin()) - 1;
    query.push_back(q);
    page.push_back((int32_t)p);
    db_id.push_back((int32_t)(t - pl.page_first[p]));
  };
  for (int64_t t : pl.every) add(-1, t);
  for (size_t k = 0; k < ids.size(); k++)
    for (int64_t t : pl.of_query[(size_t)ids[k]]) add((int32_t)k, t);
  prb_pairmask *m = nullptr;
  if (prb_pairmask_create(c, qb, db, &m) || prb_pairmask_allow(m, (int64_t)query.size(), query.data(), page.data(), db_id.data()))
    die(std::string("Error: ") + prb_last_error());
  return m;
}

int env_int(const char *a, const char *b, int dflt) {
  const char *e = std::getenv(a);
  if (!e && b) e = std::getenv(b);
  return e ? std::atoi(e) : dflt;
}

// WORLD_SIZE / RANK, the refusals of rank mode and its share of the CPUs; returns the devices of this process' workers
std::vector<int> rank_setup(Run &r) {
  const Args &a = r.a;
  std::vector<int> devices;
  if (const char *env = std::getenv("PRB_DEVICES")) {
    for (const char *p = env; *p;) {
      devices.push_back(std::atoi(p));
      while (*p && *p != ',') p++;
      if (*p == ',') p++;
    }
  }
  r.world = std::max(1, env_int("WORLD_SIZE", "OMPI_COMM_WORLD_SIZE", 1));
  r.rank = env_int("RANK", "OMPI_COMM_WORLD_RANK", 0);
  r.rank_mode = r.world > 1 || std::getenv("PRB_FORCE_COMM") != nullptr;
  if (r.rank < 0 || r.rank >= r.world) die("Error: RANK outside WORLD_SIZE");
  for (int s = kSwitches - 1; s >= 0 && r.rank_mode; s--)
    if (a.given[s] && kSwitchTable[s].not_in_rank_mode)
      die("Error: " + described(s) + " is not supported with one process per GPU (WORLD_SIZE > 1); use PRB_DEVICES=0,1,.. in one process");
  if (r.rank_mode) {
    const int local = env_int("LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", r.rank);
    const int dev = devices.empty() ? local : devices[(size_t)local % devices.size()];
    devices.assign(1, dev);
    // The ranks of a node share its CPUs: every rank runs suffix arrays + a seed DFS, rank 0 alone writes the lines of all
    // of them.  Unless the user says otherwise: half of the CPUs split over the ranks for the former, the other half for
    // rank 0's formatting (WORLD_SIZE counts ranks on other nodes too - then this errs on the small side).
    const int budget = prb_cpu_budget();
    if (r.world > 1) {
      setenv("PRB_HOST_THREADS", std::to_string(std::max(2, std::min(32, budget / (2 * r.world)))).c_str(), 0);
      if (r.rank == 0) setenv("PRB_FORMAT_THREADS", std::to_string(std::max(2, std::min(32, budget / 2))).c_str(), 0);
    }
  }
  if (devices.empty()) devices.push_back(0);
  return devices;
}

// PRB_SPLIT: one of kSplitNames; anything else is refused here, before any GPU work, the message from the same list
enum SplitKnob { kSplitAuto, kSplitQueries, kSplitPages, kSplitKnobs };
constexpr const char *kSplitNames[kSplitKnobs] = {"auto", "queries", "pages"};
void split_setup(Run &r) {
  const char *e = std::getenv("PRB_SPLIT");
  r.split_given = e != nullptr;
  r.split_knob = kSplitAuto;
  if (!e) return;
  for (int k = 0; k < kSplitKnobs; k++)
    if (std::strcmp(e, kSplitNames[k]) == 0) {
      r.split_knob = k;
      return;
    }
  std::string names;
  for (int k = 0; k < kSplitKnobs; k++) names += std::string(k ? (k + 1 < kSplitKnobs ? ", " : " or ") : "") + kSplitNames[k];
  die("Error: PRB_SPLIT needs one of " + names + " (got \"" + e + "\")");
}

// a worker per device: its context, a second one for the batch prepared ahead, the database
void open_workers(Run &r, const std::vector<int> &devices) {
  r.workers.resize(devices.size());
  const bool prefetch = !std::getenv("PRB_NO_PREFETCH");
  for (size_t k = 0; k < devices.size(); k++) {
    Worker &w = r.workers[k];
    w.device = devices[k];
    if (prb_ctx_create(devices[k], nullptr, &w.ctx)) die(std::string("Error: ") + prb_last_error());
    if (prefetch && prb_ctx_create(devices[k], nullptr, &w.prep_ctx)) die(std::string("Error: ") + prb_last_error());
    if (prb_db_open(w.ctx, r.a.db.c_str(), &w.db)) die(prb_last_error());
    if (r.a.mode == OutputMode::kTargets && prb_targetset_create(w.ctx, w.db, r.a.targets, &w.targets)) die(prb_last_error());
    if (r.a.mode == OutputMode::kCoverage && prb_covset_create(w.ctx, w.db, &w.coverage)) die(prb_last_error());
    if ((r.a.mode == OutputMode::kFeatures || r.a.mode == OutputMode::kFeatureNull || r.a.mode == OutputMode::kFeatureRank) &&
        prb_annot_create(w.ctx, w.db, (int64_t)r.annot.page.size(), r.annot.page.data(), r.annot.db_id.data(), r.annot.start.data(),
                         r.annot.end.data(), &w.annot))
      die(std::string("Error: ") + prb_last_error());
    if (r.a.mode == OutputMode::kGroupRank && prb_grouprank_create(w.ctx, (int32_t)r.groups.names.size(), r.a.grouprank, &w.grouprank))
      die(prb_last_error());
    if (r.a.mode == OutputMode::kFeatureRank) {
      if (const int rc = prb_featrank_create(w.ctx, w.annot, r.a.featrank, &w.featrank))
        die(rc == PRB_ERR_NOMEM ? std::string("Error: ") + prb_last_error() + "; lower -B" : std::string(prb_last_error()));
    }
  }
}

// the communicator of the ranks, its id exchanged through the rendezvous file
prb_comm *join_ranks(const Run &r) {
  // one file name per launch where the launcher names the launch (torchrun: TORCHELASTIC_RUN_ID; Open MPI: its job id;
  // or PRB_RUN_ID), else per MASTER_PORT
  std::string token;
  for (const char *k : {"PRB_RUN_ID", "TORCHELASTIC_RUN_ID", "OMPI_MCA_ess_base_jobid", "PMIX_NAMESPACE", "MASTER_PORT"})
    if (const char *e = std::getenv(k); e && *e && std::strcmp(e, "none") != 0) {
      token = e;
      break;
    }
  for (char &ch : token)
    if (!std::isalnum((unsigned char)ch) && ch != '-' && ch != '_') ch = '_';
  const std::string path = (r.a.tmp.empty() ? r.a.out : r.a.tmp + "/prb") + ".rccl_id." + (token.empty() ? "0" : token);
  Rendezvous rdv;
  rdv.begin(path, r.world, r.rank);
  prb_comm *comm = nullptr;
  if (prb_comm_create(r.workers[0].ctx, r.world, r.rank, rdv.id, &comm)) die(std::string("Error: ") + prb_last_error());
  rdv.end();
  return comm;
}

// what the output needs to know about the database: its parameters and the sequences of every page
void read_seq_tables(Run &r) {
  const prb_db *db = r.workers[0].db;
  int hash_size = 0;
  prb_db_info(db, &hash_size, &r.repeat_flag, &r.W, &r.delta, &r.npages);
  r.tabs.resize((size_t)r.npages);
  for (int p = 0; p < r.npages; p++) {
    int32_t nseq = 0;
    int64_t nchars = 0;
    prb_db_page_info(db, p, &nseq, &nchars);
    SeqTable &t = r.tabs[p];
    t.names.resize(nseq);
    t.len.resize(nseq);
    t.len_unmasked.resize(nseq);
    t.start_pos.resize(nseq);
    for (int32_t i = 0; i < nseq; i++) {
      t.names[i] = prb_db_seq_name(db, p, i);
      prb_db_seq_lengths(db, p, i, &t.len[i], &t.len_unmasked[i], &t.start_pos[i]);
    }
  }
}

// MergeOutput header, rna_interaction_search.cpp:445-463
std::string header_text(const Run &r) {
  const Args &a = r.a;
  std::string header = "RIblast ris result\n";
  char buf[256];
  header += "input:" + a.in + ",database:" + a.db;
  std::snprintf(buf, sizeof buf,
                ",RepeatFlag:%d,MaximalSpan:%d,MinAccessibleLength:%d,MaxSeedLength:%d,"
                "InteractionEnergyThreshold:%g,HybridEnergyThreshold:%g,FinalThreshold:%g,DropOutLengthWoGap:%d,"
                "DropOutLengthWGap:%d\n",
                r.repeat_flag, r.W, r.delta, a.o.max_seed_length, a.o.interaction_threshold, a.o.hybrid_threshold,
                a.o.final_threshold, a.o.drop_out_wo_gap, a.o.drop_out_w_gap);
  header += buf;
  switch (a.mode) {
  case OutputMode::kCoverage:
    return header + "Id,Target name,Target Length,Start,End,Hits,Max Hits,Max Queries,Peak,Minimum Interaction Energy,Query name,"
                    "Query Length,BasePair\n";
  case OutputMode::kProfile:
    return header + "Id,Query name,Query Length,Position,Hits,Targets,Minimum Interaction Energy,Target name,Target Length,BasePair\n";
  case OutputMode::kSummary:
  case OutputMode::kTop:
  case OutputMode::kTargets:
    return header + "Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
                    "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair\n";
  case OutputMode::kGroups:
  case OutputMode::kGroupRank:
    return header + "Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
                    "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair, Group, Members, Group Size, "
                    "Group Hits\n";
  case OutputMode::kFeatures:
  case OutputMode::kFeatureRank:
    return header + "Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
                    "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair, Feature, Feature Range, "
                    "Inside\n";
  case OutputMode::kFeatureNull:
    return header + "Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
                    "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair, Feature, Feature Range, "
                    "Inside, Decoys, Null Hits, Null LE, Null Minimum Energy, P Value\n";
  case OutputMode::kGroupNull:
    return header + "Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
                    "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair, Group, Members, Group Size, "
                    "Group Hits, Decoys, Null Hits, Null LE, Null Minimum Energy, P Value\n";
  case OutputMode::kNull:
    return header + "Id,Query name, Query Length, Target name, Target Length, Hits, Minimum Interaction Energy, "
                    "Sum of Interaction Energies, Accessibility Energy, Hybridization Energy, BasePair, Decoys, Null Hits, Null LE, "
                    "Null Minimum Energy, P Value" + (a.given[kQValue] ? ", Tests, Rank, Q Value\n" : "\n");
  case OutputMode::kScored:
    return header + "Id,Query name, Query Length, Target name, Target Length, Accessibility Energy, Hybridization Energy, "
                    "Interaction Energy, BasePair, Decoys, Null LE, Rank, E Value, Q Value\n";
  case OutputMode::kHits:
  case OutputMode::kTopHits: break;
  }
  return header + "Id,Query name, Query Length, Target name, Target Length, Accessibility Energy, Hybridization Energy, "
                  "Interaction Energy, BasePair\n";
}

// the output file (rank 0's; the other ranks write nowhere) with its header
void open_output(Run &r) {
  r.out = std::fopen(r.rank == 0 ? r.a.out.c_str() : "/dev/null", r.a.binary() ? "wb" : "w");
  if (!r.out) die("Error: can't open output_file: " + r.a.out);
  const std::string header = header_text(r);
  if (r.a.binary()) write_binary_head(r.out, r.a.o.output_style, header, r.tabs);
  else put(r.out, header.data(), header.size());
  if (std::fflush(r.out)) die("Error: can't write the output file");
}

void plan_batches(Run &r) {
  // Queries per batch: PRB_BATCH, else large batches (full launches of the small-list kernels) but at least four per
  // worker / rank, so that every GPU has work and the last round is short (the reference deals single queries)
  const char *benv = std::getenv("PRB_BATCH");
  const size_t consumers = r.rank_mode ? (size_t)r.world : r.workers.size(), nseq = r.seqs.size();
  r.batch = benv ? (size_t)std::max(1, std::atoi(benv))
                 : std::max<size_t>(16, std::min<size_t>(2048, (nseq + 4 * consumers - 1) / (4 * consumers)));
  // longest first (stable: equal lengths keep their FASTA order), then batches in that order
  r.order.resize(nseq);
  std::iota(r.order.begin(), r.order.end(), (size_t)0);
  std::stable_sort(r.order.begin(), r.order.end(), [&](size_t x, size_t y) { return r.seqs[x].size() > r.seqs[y].size(); });
  r.nb = (nseq + r.batch - 1) / r.batch;
  // a job of the writer is a batch - or, with one process per GPU, a round of WORLD_SIZE batches gathered on rank 0
  r.njobs = r.rank_mode ? (r.nb + r.world - 1) / r.world : r.nb;
}

// Whole batches to the workers, or the pages of every batch?  Pages only in one process with two workers or more and
// a database of two pages or more: when asked for, or - auto - when there are fewer batches than workers.
void plan_split(Run &r) {
  const bool can = !r.rank_mode && r.workers.size() >= 2 && r.npages >= 2 && !runs_decoys(r.a.mode);
  r.split_pages = can && (r.split_knob == kSplitPages || (r.split_knob == kSplitAuto && r.nb < r.workers.size()));
}

// encode + suffix arrays + accessibilities of batch b under context c; the seed search against seed_page is begun
// beside them (none if it is negative)
Prepared prepare_batch(const Run &r, prb_ctx *c, const prb_db *db, size_t b, int seed_page = 0) {
  const std::vector<size_t> idx = r.batch_idx(b);
  std::string cat;
  std::vector<int64_t> off(idx.size() + 1, 0);
  for (size_t k = 0; k < idx.size(); k++) {
    cat += r.seqs[idx[k]];
    off[k + 1] = (int64_t)cat.size();
  }
  Prepared p;
  if (prb_qbatch_create(c, (int32_t)idx.size(), cat.data(), off.data(), r.repeat_flag, &p.qb)) die(prb_last_error());
  // the seed DFS against the first page needs no GPU: it runs on host threads beside the accessibilities (and,
  // for a batch prepared ahead, beside the previous batch's search)
  if (db && seed_page >= 0 && prb_qbatch_seed_search_begin(c, p.qb, db, seed_page, &r.a.o)) die(prb_last_error());
  if (prb_qbatch_accessibility(c, p.qb, r.W, r.delta)) die(prb_last_error());
  p.qlen_unmasked.resize(idx.size());
  for (size_t q = 0; q < idx.size(); q++) p.qlen_unmasked[q] = prb_qbatch_length_unmasked(p.qb, (int32_t)q);
  p.ids.assign(idx.begin(), idx.end());
  if (r.a.have_pairlist) p.mask = batch_mask(r, c, p.qb, db, p.ids);
  return p;
}
// a searched batch's queries and mask let go
void release_batch(Prepared &p) {
  prb_qbatch_destroy(p.qb);
  prb_pairmask_free(p.mask);
  p.qb = nullptr;
  p.mask = nullptr;
}

// -t -n, -q, -k: a table per batch; every page is searched and merged into it on the device by `search`, then one copy
// of its records to the host by `finish`
template <class T> struct TableOps {
  int (*search)(prb_ctx *, prb_qbatch *, prb_db *, int32_t, const prb_ris_opts *, T *);
  int (*merge)(prb_ctx *, T *, T *); // another worker's table of the same batch into this one (a team, run_team)
  int (*finish)(prb_ctx *, T *);
};
const TableOps<prb_topset> kTopOps = {prb_search_page_top, prb_topset_merge, prb_topset_finish};
const TableOps<prb_profset> kProfOps = {prb_search_page_profile, prb_profset_merge, prb_profset_finish};
const TableOps<prb_tophits> kTopHitsOps = {prb_search_page_tophits, prb_tophits_merge, prb_tophits_finish};

// the run's options with a batch's own mask (-L; a decoy piece's)
prb_ris_opts opts_with(const Run &r, const prb_pairmask *mask) {
  prb_ris_opts o = r.a.o;
  o.allowed_pairs = mask;
  return o;
}

// -t -G: the empty group table of a batch
Handle<prb_groupset> create_groupset(const Run &r, Worker &w, prb_qbatch *qb) {
  std::vector<const int32_t *> maps;
  for (const auto &m : r.groups.of_page) maps.push_back(m.data());
  prb_groupset *t = nullptr;
  const int rc = prb_groupset_create(w.ctx, qb, w.db, maps.data(), (int32_t)r.groups.names.size(), &t);
  Handle<prb_groupset> gs(t);
  if (rc == PRB_ERR_NOMEM)
    die(std::string("Error: ") + prb_last_error() + "; lower PRB_BATCH (queries per batch: " + std::to_string(r.batch) + ")");
  if (rc) die(prb_last_error());
  return gs;
}

// the empty table of a batch, by mode (nothing for the modes that have none: the run's tables, the page sets - and
// runs_decoys, which never come here), in res
void create_table(const Run &r, Worker &w, prb_qbatch *qb, BatchResult &res) {
  const Args &a = r.a;
  int rc = 0;
  switch (a.mode) {
  case OutputMode::kTop: {
    prb_topset *t = nullptr;
    rc = prb_topset_create(w.ctx, qb, a.top, &t);
    res.top.reset(t);
    break;
  }
  case OutputMode::kProfile: {
    prb_profset *t = nullptr;
    rc = prb_profset_create(w.ctx, qb, &t);
    res.prof.reset(t);
    break;
  }
  case OutputMode::kTopHits: {
    prb_tophits *t = nullptr;
    rc = prb_tophits_create(w.ctx, qb, a.tophits, &t);
    res.tophits.reset(t);
    break;
  }
  case OutputMode::kFeatures:
  case OutputMode::kFeatureRank: { // (-B: the batch's feature table, merged into the worker's)
    prb_featset *t = nullptr;
    rc = prb_featset_create(w.ctx, qb, w.annot, &t);
    res.features.reset(t);
    break;
  }
  case OutputMode::kGroups:
  case OutputMode::kGroupRank: res.groups = create_groupset(r, w, qb); break; // (-R: the batch's group table, merged into the worker's)
  default: break; // (kTargets, kCoverage: the worker's own table, for the whole run - open_workers)
  }
  if (rc) die(prb_last_error());
}

// one page of a prepared batch searched: into the table of `mine` (-r: into the worker's), or - a hit set or a pair set -
// into slot `page` of `out`
void search_one_page(const Run &r, Worker &w, const Prepared &p, int page, BatchResult &mine, BatchResult &out) {
  prb_qbatch *qb = p.qb;
  const prb_ris_opts o = opts_with(r, p.mask);
  int rc = 0;
  switch (r.a.mode) {
  case OutputMode::kTargets: rc = prb_search_page_targets(w.ctx, qb, w.db, page, &o, p.ids.data(), w.targets); break;
  case OutputMode::kCoverage: rc = prb_search_page_coverage(w.ctx, qb, w.db, page, &o, p.ids.data(), w.coverage); break;
  case OutputMode::kTop: rc = kTopOps.search(w.ctx, qb, w.db, page, &o, mine.top.get()); break;
  case OutputMode::kProfile: rc = kProfOps.search(w.ctx, qb, w.db, page, &o, mine.prof.get()); break;
  case OutputMode::kTopHits: rc = kTopHitsOps.search(w.ctx, qb, w.db, page, &o, mine.tophits.get()); break;
  case OutputMode::kFeatures:
  case OutputMode::kFeatureRank: rc = prb_search_page_features(w.ctx, qb, w.db, page, &o, mine.features.get()); break;
  case OutputMode::kGroups:
  case OutputMode::kGroupRank: rc = prb_search_page_groups(w.ctx, qb, w.db, page, &o, mine.groups.get()); break;
  case OutputMode::kSummary: {
    prb_pairset *ps = nullptr;
    rc = prb_search_page_summary(w.ctx, qb, w.db, page, &o, &ps);
    out.pair_pages[(size_t)page].reset(ps);
    break;
  }
  case OutputMode::kHits: {
    prb_hitset *hs = nullptr;
    rc = prb_search_page(w.ctx, qb, w.db, page, &o, 3, &hs);
    out.pages[(size_t)page].reset(hs);
    break;
  }
  default: break; // (runs_decoys: never here)
  }
  if (rc) die(prb_last_error());
}

// the table of `mine` - with the tables of `others` merged into it first - to the host: one copy of its records; -R, -B:
// into the worker's table of the run under the input positions of the batch `p`, on the device, and dropped
void finish_table(const Run &r, Worker &w, const Prepared &p, BatchResult &mine, const std::vector<BatchResult *> &others = {}) {
  auto run = [&](auto ops, auto member) {
    for (BatchResult *o : others)
      if (ops.merge(w.ctx, (mine.*member).get(), (o->*member).get())) die(prb_last_error());
    if (ops.finish(w.ctx, (mine.*member).get())) die(prb_last_error());
  };
  switch (r.a.mode) {
  case OutputMode::kTop: run(kTopOps, &BatchResult::top); break;
  case OutputMode::kProfile: run(kProfOps, &BatchResult::prof); break;
  case OutputMode::kTopHits: run(kTopHitsOps, &BatchResult::tophits); break;
  case OutputMode::kGroups: // (its finish takes the -n of the run: 0 without one)
    for (BatchResult *o : others)
      if (prb_groupset_merge(w.ctx, mine.groups.get(), o->groups.get())) die(prb_last_error());
    if (prb_groupset_finish(w.ctx, mine.groups.get(), r.a.given[kN] ? r.a.top : 0)) die(prb_last_error());
    break;
  case OutputMode::kFeatures:
    for (BatchResult *o : others)
      if (prb_featset_merge(w.ctx, mine.features.get(), o->features.get())) die(prb_last_error());
    if (r.a.given[kFN] ? prb_featset_finish_top(w.ctx, mine.features.get(), r.a.feattop) : prb_featset_finish(w.ctx, mine.features.get()))
      die(prb_last_error());
    break;
  case OutputMode::kGroupRank: // (a group's members may lie on any page: only the batch's whole group table is ranked)
    for (BatchResult *o : others)
      if (prb_groupset_merge(w.ctx, mine.groups.get(), o->groups.get())) die(prb_last_error());
    if (prb_grouprank_add_groupset(w.ctx, w.grouprank, mine.groups.get(), p.ids.data())) die(prb_last_error());
    mine.groups.reset();
    break;
  case OutputMode::kFeatureRank: // (every identifier is merged once: only the batch's whole feature table is ranked)
    for (BatchResult *o : others)
      if (prb_featset_merge(w.ctx, mine.features.get(), o->features.get())) die(prb_last_error());
    if (prb_featrank_add_featset(w.ctx, w.featrank, mine.features.get(), p.ids.data())) die(prb_last_error());
    mine.features.reset();
    break;
  default: break; // (no table of the batch's own to finish: create_table)
  }
}

// a result with a slot per page for the modes that keep the pages apart
BatchResult empty_result(const Run &r) {
  BatchResult res;
  res.mode = r.a.mode;
  if (r.a.mode == OutputMode::kHits) res.pages.resize((size_t)r.npages);
  if (r.a.mode == OutputMode::kSummary) res.pair_pages.resize((size_t)r.npages);
  return res;
}

// -r, -c, -R, -B: the lines are written at the end of the run, with every query's unmasked length by its place in the input
void note_target_queries(const Run &r, Worker &w, const Prepared &p) {
  if (r.a.mode != OutputMode::kTargets && r.a.mode != OutputMode::kCoverage && r.a.mode != OutputMode::kGroupRank &&
      r.a.mode != OutputMode::kFeatureRank)
    return;
  for (size_t q = 0; q < p.ids.size(); q++) w.target_qlen.emplace_back(p.ids[q], p.qlen_unmasked[q]);
}

// ---- -z, -P, -E: a batch and its decoys (runs_decoys) ------------------------------------------------
// One piece of a batch's decoys, ready to be searched: at most the batch size of them
struct DecoyPiece {
  std::vector<int32_t> owner, decoy, ids; // per decoy: its query's place in the batch, its number, its query's place in the input file
  Handle<prb_qbatch> qb;                  // the shuffles, with their suffix arrays and accessibilities
  Handle<prb_pairmask> mask;              // what the mode's body restricts their search to, if anything
};

// The decoys of a prepared batch - N shuffles of every query (prb_shuffle_sequence under the run's seed, the query's place
// in the input file and the decoy's number), made on host threads -, query by query and decoy by decoy, in pieces of at
// most the batch size: each piece gets its suffix arrays and accessibilities, goes to the mode's `body` - which makes
// the piece's mask, if it wants one, and searches the piece against every page -, and is let go of with its mask.
// The general form takes the decoys [d_lo, d_hi) of the queries `queries` of the batch (ascending places in it) - one
// round of `-H` for the queries that still have live pairs -, in the same order.
template <class Body>
void for_decoy_pieces(const Run &r, Worker &w, const Prepared &p, const std::vector<int32_t> &queries, int32_t d_lo, int32_t d_hi, Body body) {
  const size_t nd = (size_t)(d_hi - d_lo), total = queries.size() * nd;
  for (size_t d0 = 0; d0 < total; d0 += r.batch) {
    const size_t m = std::min(total, d0 + r.batch) - d0;
    DecoyPiece dp;
    dp.owner.resize(m);
    dp.decoy.resize(m);
    dp.ids.resize(m);
    std::vector<int64_t> off(m + 1, 0);
    for (size_t k = 0; k < m; k++) {
      dp.owner[k] = queries[(d0 + k) / nd];
      dp.decoy[k] = d_lo + (int32_t)((d0 + k) % nd);
      dp.ids[k] = p.ids[(size_t)dp.owner[k]];
      off[k + 1] = off[k] + (int64_t)r.seqs[(size_t)dp.ids[k]].size();
    }
    std::string cat((size_t)off[m], '\0');
    bool shuffled = true;
#pragma omp parallel for schedule(dynamic, 1) num_threads(std::max(1, prb_host_threads_default()))
    for (size_t k = 0; k < m; k++) {
      const std::string &seq = r.seqs[(size_t)dp.ids[k]];
      if (prb_shuffle_sequence(seq.data(), (int32_t)seq.size(), r.a.shuffle_seed, (int64_t)dp.ids[k], dp.decoy[k], &cat[(size_t)off[k]])) {
#pragma omp atomic write
        shuffled = false;
      }
    }
    if (!shuffled) die(std::string("Error: ") + prb_last_error());
    prb_qbatch *dqb = nullptr;
    if (prb_qbatch_create(w.ctx, (int32_t)m, cat.data(), off.data(), r.repeat_flag, &dqb)) die(prb_last_error());
    dp.qb.reset(dqb);
    if (prb_qbatch_accessibility(w.ctx, dqb, r.W, r.delta)) die(prb_last_error());
    body(dp);
  }
}
template <class Body> void for_decoy_pieces(const Run &r, Worker &w, const Prepared &p, Body body) {
  std::vector<int32_t> all(p.ids.size());
  std::iota(all.begin(), all.end(), 0);
  for_decoy_pieces(r, w, p, all, 0, r.a.decoys, body);
}

// PRB_NULL_MASK=0: -z and -P search their decoys without a mask of the mode's own
bool null_mask_wanted() {
  const char *menv = std::getenv("PRB_NULL_MASK");
  return !(menv && std::atoi(menv) == 0);
}
// A piece's masks: the one of the targets that each_target(k, add) names for decoy k with add(page, db_id), and - under
// -L - the one of its owners' listed pairs
template <class EachTarget> void mask_piece(Worker &w, DecoyPiece &dp, EachTarget each_target) {
  std::vector<int32_t> mq, mp, md;
  for (size_t k = 0; k < dp.owner.size(); k++)
    each_target(k, [&](int32_t page, int32_t db_id) {
      mq.push_back((int32_t)k);
      mp.push_back(page);
      md.push_back(db_id);
    });
  prb_pairmask *m = nullptr;
  const int rc = prb_pairmask_create(w.ctx, dp.qb.get(), w.db, &m);
  dp.mask.reset(m);
  if (rc || prb_pairmask_allow(m, (int64_t)mq.size(), mq.data(), mp.data(), md.data())) die(std::string("Error: ") + prb_last_error());
}
void mask_piece_by_list(const Run &r, Worker &w, DecoyPiece &dp) {
  if (r.a.have_pairlist) dp.mask.reset(batch_mask(r, w.ctx, dp.qb.get(), w.db, dp.ids));
}

// The null table finished: as it is, or - with -Q - with the Benjamini-Hochberg figures of its pairs ranked on the device
// (prb_nullset_finish_fdr).  A query's tests are the targets it was searched against: every target of the database, or
// under -L the distinct targets that the list names for it or for every query - the list's own count, on the host already
// (a query without any has no pair either: 1).
void finish_null_table(const Run &r, Worker &w, const Prepared &p, prb_nullset *ns) {
  if (!r.a.given[kQValue]) {
    if (prb_nullset_finish(w.ctx, ns)) die(prb_last_error());
    return;
  }
  std::vector<int64_t> tests;
  if (p.mask) {
    tests.assign(p.ids.size(), 0);
    for (size_t q = 0; q < tests.size(); q++) {
      std::vector<int64_t> listed = r.list.every;
      const std::vector<int64_t> &own = r.list.of_query[(size_t)p.ids[q]];
      listed.insert(listed.end(), own.begin(), own.end());
      std::sort(listed.begin(), listed.end());
      tests[q] = std::max<int64_t>(std::unique(listed.begin(), listed.end()) - listed.begin(), 1);
    }
  }
  if (prb_nullset_finish_fdr(w.ctx, ns, p.mask ? tests.data() : nullptr)) die(prb_last_error());
}

// -t -z N: the real batch against every page into a null table of its own, then its decoys against every page.  Unless
// PRB_NULL_MASK=0, a piece is searched under a pair mask that allows each decoy the observed targets of its owner only
// (under -L those are listed pairs already): the real batch's records come to the host for that
// (prb_search_page_summary) and go into the table from there (prb_nullset_observe); without the mask - none at all, also
// under -L - they never leave the device (prb_search_page_observed).
// -t -z N -H H [-D R]: the real batch against every page into the null table on the device (prb_search_page_observed: no
// record comes to the host), then the decoys round by round: the decoys [b, b + R) of the queries that still have live
// pairs, each piece - unless PRB_NULL_MASK=0 - under the mask of its owners' live pairs, which the device makes from the
// table (prb_pairmask_create_live; under -L live pairs are listed pairs already); at the round's end the pairs with
// NullLE >= H retire (prb_nullset_retire), and a query left without live pairs gets no further decoys - no shuffle, no
// suffix array, no accessibility.  One line on stderr says how many pairs were live after each round.
BatchResult search_seqnull_batch(const Run &r, Worker &w, Prepared &p) {
  BatchResult res = empty_result(r);
  const bool masked = null_mask_wanted();
  const size_t nq = p.ids.size();
  const int32_t N = r.a.decoys;
  prb_nullset *ns = nullptr;
  if (prb_nullset_create(w.ctx, p.qb, w.db, N, &ns)) die(prb_last_error());
  res.null.reset(ns);
  const prb_ris_opts o = opts_with(r, p.mask);
  for (int page = 0; page < r.npages; page++)
    if (prb_search_page_observed(w.ctx, p.qb, w.db, page, &o, ns)) die(prb_last_error());
  std::vector<int32_t> queries(nq);
  std::iota(queries.begin(), queries.end(), 0);
  std::vector<int64_t> live(nq, 0);
  std::string after;
  for (int32_t lo = 0, hi; lo < N && !queries.empty(); lo = hi) {
    hi = std::min(N, lo + r.a.round);
    for_decoy_pieces(r, w, p, queries, lo, hi, [&](DecoyPiece &dp) {
      if (masked) {
        prb_pairmask *m = nullptr;
        const int rc = prb_pairmask_create_live(w.ctx, ns, dp.qb.get(), dp.owner.data(), (int32_t)dp.owner.size(), &m);
        dp.mask.reset(m);
        if (rc) die(std::string("Error: ") + prb_last_error());
      }
      const prb_ris_opts od = opts_with(r, dp.mask.get());
      for (int page = 0; page < r.npages; page++)
        if (prb_search_page_decoys(w.ctx, dp.qb.get(), w.db, page, &od, dp.owner.data(), dp.decoy.data(), ns)) die(prb_last_error());
    });
    if (prb_nullset_retire(w.ctx, ns, r.a.retire_le, hi, live.data())) die(prb_last_error());
    queries.clear();
    for (size_t q = 0; q < nq; q++)
      if (live[q] > 0) queries.push_back((int32_t)q);
    after += (after.empty() ? "" : ", ") + std::to_string(hi) + ": " + std::to_string(std::accumulate(live.begin(), live.end(), (int64_t)0));
  }
  std::fprintf(stderr, "sequential null: %zu queries, live pairs after decoy %s; queries without live pairs: %zu\n", nq, after.c_str(), nq - queries.size());
  finish_null_table(r, w, p, ns);
  release_batch(p);
  return res;
}

BatchResult search_null_batch(const Run &r, Worker &w, Prepared &p) {
  if (r.a.given[kH]) return search_seqnull_batch(r, w, p);
  BatchResult res = empty_result(r);
  const bool masked = null_mask_wanted();
  const size_t nq = p.ids.size();
  prb_nullset *ns = nullptr;
  if (prb_nullset_create(w.ctx, p.qb, w.db, r.a.decoys, &ns)) die(prb_last_error());
  res.null.reset(ns);
  const prb_ris_opts o = opts_with(r, p.mask);
  std::vector<std::vector<std::pair<int32_t, int32_t>>> observed(nq); // per query: its (page, db_id)
  for (int page = 0; page < r.npages; page++) {
    if (!masked) {
      if (prb_search_page_observed(w.ctx, p.qb, w.db, page, &o, ns)) die(prb_last_error());
      continue;
    }
    prb_pairset *raw = nullptr;
    if (prb_search_page_summary(w.ctx, p.qb, w.db, page, &o, &raw)) die(prb_last_error());
    const Handle<prb_pairset> ps(raw);
    const prb_pair_summary *rec = prb_pairset_pairs(raw);
    const int64_t n = prb_pairset_size(raw);
    for (int64_t i = 0; i < n; i++) {
      if (rec[i].query < 0 || (size_t)rec[i].query >= nq) die("Error: bad record in a batch's pair summaries");
      observed[(size_t)rec[i].query].emplace_back((int32_t)page, rec[i].db_id);
    }
    if (prb_nullset_observe(w.ctx, ns, page, rec, n)) die(prb_last_error());
  }
  for_decoy_pieces(r, w, p, [&](DecoyPiece &dp) {
    if (masked)
      mask_piece(w, dp, [&](size_t k, auto add) {
        for (const auto &[page, db_id] : observed[(size_t)dp.owner[k]]) add(page, db_id);
      });
    const prb_ris_opts od = opts_with(r, dp.mask.get());
    for (int page = 0; page < r.npages; page++)
      if (prb_search_page_decoys(w.ctx, dp.qb.get(), w.db, page, &od, dp.owner.data(), dp.decoy.data(), ns)) die(prb_last_error());
  });
  finish_null_table(r, w, p, ns);
  release_batch(p);
  return res;
}

// -t -G FILE -P N: the real batch against every page into a group table, which is finished - under the run's -n - into a
// group null table: nothing comes to the host but the kept records.  Then the decoys, each piece against every page
// between prb_gnullset_begin and prb_gnullset_end.  Unless PRB_NULL_MASK=0, a piece is searched under a pair mask that
// allows each decoy the members of its owner's kept groups only - under -L those of them that are listed for the owner;
// with PRB_NULL_MASK=0, under -L, every pair listed for the owner (the statistic runs over the listed targets either way).
BatchResult search_gnull_batch(const Run &r, Worker &w, Prepared &p) {
  BatchResult res = empty_result(r);
  const Args &a = r.a;
  const bool masked = null_mask_wanted();
  const size_t nq = p.ids.size();
  Handle<prb_groupset> real = create_groupset(r, w, p.qb);
  const prb_ris_opts o = opts_with(r, p.mask);
  for (int page = 0; page < r.npages; page++)
    if (prb_search_page_groups(w.ctx, p.qb, w.db, page, &o, real.get())) die(prb_last_error());
  prb_gnullset *gn = nullptr;
  if (prb_gnullset_create(w.ctx, real.get(), a.given[kN] ? a.top : 0, a.decoys, &gn)) die(prb_last_error());
  res.gnull.reset(gn);
  // per query its kept groups, and - under -L - its listed targets, numbered page by page, ascending
  std::vector<std::vector<int32_t>> kept(nq);
  {
    const prb_group_pair *rec = prb_groupset_pairs(real.get());
    const int64_t n = prb_groupset_size(real.get());
    for (int64_t i = 0; i < n; i++) {
      if (rec[i].s.query < 0 || (size_t)rec[i].s.query >= nq || rec[i].group < 0 || (size_t)rec[i].group >= r.groups.members.size())
        die("Error: bad record in the group table");
      kept[(size_t)rec[i].s.query].push_back(rec[i].group);
    }
  }
  real.reset();
  std::vector<int64_t> page_first(1, 0);
  for (const auto &m : r.groups.of_page) page_first.push_back(page_first.back() + (int64_t)m.size());
  std::vector<std::vector<int64_t>> listed(a.have_pairlist && masked ? nq : 0);
  for (size_t q = 0; q < listed.size(); q++) {
    listed[q] = r.list.every;
    const std::vector<int64_t> &own = r.list.of_query[(size_t)p.ids[q]];
    listed[q].insert(listed[q].end(), own.begin(), own.end());
    std::sort(listed[q].begin(), listed[q].end());
  }
  for_decoy_pieces(r, w, p, [&](DecoyPiece &dp) {
    if (masked)
      mask_piece(w, dp, [&](size_t k, auto add) {
        for (int32_t g : kept[(size_t)dp.owner[k]])
          for (const auto &[page, db_id] : r.groups.members[(size_t)g]) {
            if (a.have_pairlist) {
              const std::vector<int64_t> &l = listed[(size_t)dp.owner[k]];
              if (!std::binary_search(l.begin(), l.end(), page_first[(size_t)page] + db_id)) continue;
            }
            add(page, db_id);
          }
      });
    else
      mask_piece_by_list(r, w, dp);
    const prb_ris_opts od = opts_with(r, dp.mask.get());
    if (prb_gnullset_begin(w.ctx, gn, dp.owner.data(), dp.decoy.data(), (int32_t)dp.owner.size())) die(std::string("Error: ") + prb_last_error());
    for (int page = 0; page < r.npages; page++)
      if (prb_search_page_gnull(w.ctx, dp.qb.get(), w.db, page, &od, gn)) die(prb_last_error());
    if (prb_gnullset_end(w.ctx, gn)) die(prb_last_error());
  });
  if (prb_gnullset_finish(w.ctx, gn)) die(prb_last_error());
  release_batch(p);
  return res;
}

// -t -A FILE -F N: the real batch against every page into a feature table, which is finished into a feature null table:
// nothing comes to the host but the kept records.  Then the decoys, each piece against every page between
// prb_fnullset_begin and prb_fnullset_end.  Unless PRB_NULL_MASK=0, a piece is searched under a pair mask that allows each
// decoy the targets of its owner's kept records only (under -L those are listed pairs already); with PRB_NULL_MASK=0,
// under -L, every pair listed for the owner.  A query without a record has its decoys searched against nothing, and closed.
// With -N K the feature null table is made over each query's K best records (prb_fnullset_create_top), which are then all
// that "kept" means here: the mask allows a decoy the targets of those K records only.
BatchResult search_fnull_batch(const Run &r, Worker &w, Prepared &p) {
  BatchResult res = empty_result(r);
  const bool masked = null_mask_wanted();
  const size_t nq = p.ids.size();
  prb_featset *raw = nullptr;
  if (prb_featset_create(w.ctx, p.qb, w.annot, &raw)) die(prb_last_error());
  Handle<prb_featset> real(raw);
  const prb_ris_opts o = opts_with(r, p.mask);
  for (int page = 0; page < r.npages; page++)
    if (prb_search_page_features(w.ctx, p.qb, w.db, page, &o, real.get())) die(prb_last_error());
  prb_fnullset *fn = nullptr;
  if (r.a.given[kFN] ? prb_fnullset_create_top(w.ctx, real.get(), r.a.decoys, r.a.feattop, &fn) : prb_fnullset_create(w.ctx, real.get(), r.a.decoys, &fn))
    die(prb_last_error());
  res.fnull.reset(fn);
  // per query the targets of its kept records (a target comes once per feature with a record: the mask takes it again)
  std::vector<std::vector<std::pair<int32_t, int32_t>>> kept(masked ? nq : 0);
  if (masked) {
    const prb_feature_pair *rec = prb_featset_records(real.get());
    const int64_t n = prb_featset_size(real.get());
    for (int64_t i = 0; i < n; i++) {
      if (rec[i].s.query < 0 || (size_t)rec[i].s.query >= nq || rec[i].page < 0 || rec[i].page >= r.npages || rec[i].s.db_id < 0)
        die("Error: bad record in the feature table");
      std::vector<std::pair<int32_t, int32_t>> &k = kept[(size_t)rec[i].s.query];
      if (k.empty() || k.back() != std::make_pair(rec[i].page, rec[i].s.db_id)) k.emplace_back(rec[i].page, rec[i].s.db_id);
    }
  }
  real.reset();
  for_decoy_pieces(r, w, p, [&](DecoyPiece &dp) {
    if (masked)
      mask_piece(w, dp, [&](size_t k, auto add) {
        for (const auto &[page, db_id] : kept[(size_t)dp.owner[k]]) add(page, db_id);
      });
    else
      mask_piece_by_list(r, w, dp);
    const prb_ris_opts od = opts_with(r, dp.mask.get());
    if (prb_fnullset_begin(w.ctx, fn, dp.owner.data(), dp.decoy.data(), (int32_t)dp.owner.size())) die(std::string("Error: ") + prb_last_error());
    for (int page = 0; page < r.npages; page++)
      if (prb_search_page_fnull(w.ctx, dp.qb.get(), w.db, page, &od, fn)) die(prb_last_error());
    if (prb_fnullset_end(w.ctx, fn)) die(prb_last_error());
  });
  if (prb_fnullset_finish(w.ctx, fn)) die(prb_last_error());
  release_batch(p);
  return res;
}

// -k K -E M: the real batch against every page, once, into the top-N hit table and an evalset beside it; then its decoys
// against every page into the evalset's decoy list.  There is no decoy mask, whatever PRB_NULL_MASK says: the null is
// pooled over every target (under -L: over the owner's listed targets, the query's own search space).  The evalset is
// closed, the table finished, and the kept hits looked up on the device.
BatchResult search_scored_batch(const Run &r, Worker &w, Prepared &p) {
  BatchResult res = empty_result(r);
  const Args &a = r.a;
  prb_tophits *th = nullptr;
  if (prb_tophits_create(w.ctx, p.qb, a.tophits, &th)) die(prb_last_error());
  res.tophits.reset(th);
  prb_evalset *raw = nullptr;
  if (prb_evalset_create(w.ctx, p.qb, w.db, a.decoys, &raw)) die(prb_last_error());
  const Handle<prb_evalset> es(raw);
  const prb_ris_opts o = opts_with(r, p.mask);
  for (int page = 0; page < r.npages; page++)
    if (prb_search_page_scored(w.ctx, p.qb, w.db, page, &o, th, es.get())) die(prb_last_error());
  for_decoy_pieces(r, w, p, [&](DecoyPiece &dp) {
    mask_piece_by_list(r, w, dp);
    const prb_ris_opts od = opts_with(r, dp.mask.get());
    for (int page = 0; page < r.npages; page++)
      if (prb_search_page_null_hits(w.ctx, dp.qb.get(), w.db, page, &od, dp.owner.data(), dp.decoy.data(), es.get())) die(prb_last_error());
  });
  if (prb_evalset_close(w.ctx, es.get())) die(prb_last_error());
  if (prb_tophits_finish(w.ctx, th)) die(prb_last_error());
  const prb_top_hit *rec = prb_tophits_hits(th);
  const int64_t n = prb_tophits_size(th);
  std::vector<int32_t> lq((size_t)n);
  std::vector<double> le((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    lq[(size_t)i] = rec[i].h.query;
    le[(size_t)i] = rec[i].h.e_tot;
  }
  res.scores.resize((size_t)n);
  if (prb_evalset_score(w.ctx, es.get(), lq.data(), le.data(), n, res.scores.data())) die(prb_last_error());
  release_batch(p);
  return res;
}

// the search stages of a prepared batch against every page
BatchResult search_batch(const Run &r, Worker &w, Prepared &p) {
  if (r.a.mode == OutputMode::kScored) return search_scored_batch(r, w, p);
  if (r.a.mode == OutputMode::kNull) return search_null_batch(r, w, p);
  if (r.a.mode == OutputMode::kGroupNull) return search_gnull_batch(r, w, p);
  if (r.a.mode == OutputMode::kFeatureNull) return search_fnull_batch(r, w, p);
  BatchResult res = empty_result(r);
  create_table(r, w, p.qb, res);
  for (int page = 0; page < r.npages; page++) search_one_page(r, w, p, page, res, res);
  finish_table(r, w, p, res);
  note_target_queries(r, w, p);
  release_batch(p);
  return res;
}

// ---- the writer ----------------------------------------------------------------------------------
void set_queries(prb::QueryView &v, const BatchJob &job) {
  v.nq = job.names.size();
  v.names = job.names.data();
  v.qlen_unmasked = job.qlen_unmasked.data();
}
int64_t written_or_die(int64_t id) {
  if (id < 0) die("Error: can't write the output file");
  return id;
}
// the hits of a batch as binary records or as result lines; returns the next id
int64_t write_hits(const Run &r, const BatchView &v, int64_t id, LineSink &sink) {
  if (r.a.binary()) return id + write_binary_batch(v, r.out);
  return written_or_die(prb::format_batch(v, r.tabs, r.a.o.output_style, id, sink, prb::format_threads()));
}

// The kept hits come by query, then by rank, the pages mixed; the writers take hits page by page, ascending by
// query, and write a query's hits of one page in the order given.  So the records are cut where a query's next
// hit lies in a lower page, and every piece goes out as a batch of its own (one piece for a database of one page).
// -k -E: every record's score (job.res.scores, in the records' order) goes with it, behind its line.
int64_t write_tophits(const Run &r, const BatchJob &job, int64_t id, LineSink &sink) {
  const bool scored = job.res.mode == OutputMode::kScored;
  const int npages = r.npages;
  const prb_top_hit *rec = prb_tophits_hits(job.res.tophits.get());
  const int64_t n = prb_tophits_size(job.res.tophits.get());
  int64_t nbp = 0;
  const int32_t *bp = prb_tophits_basepairs(job.res.tophits.get(), &nbp);
  std::vector<std::vector<prb_hit>> hits((size_t)npages);
  std::vector<std::vector<int32_t>> pairs((size_t)npages);
  std::vector<std::vector<prb_eval_score>> scores(scored ? (size_t)npages : 0);
  if (scored && (int64_t)job.res.scores.size() != n) die("Error: the scores of the best hits do not match their records");
  for (int64_t i0 = 0; i0 < n;) {
    int64_t i1 = i0 + 1;
    while (i1 < n && !(rec[i1].h.query == rec[i1 - 1].h.query && rec[i1].page < rec[i1 - 1].page)) i1++;
    const int32_t qa = rec[i0].h.query, qz = rec[i1 - 1].h.query;
    for (auto &h : hits) h.clear();
    for (auto &p : pairs) p.clear();
    for (auto &s : scores) s.clear();
    for (int64_t i = i0; i < i1; i++) {
      prb_hit x = rec[i].h;
      if (rec[i].page < 0 || rec[i].page >= npages || x.bp_count < 0 || x.bp_offset < 0 || x.bp_offset + x.bp_count > nbp)
        die("Error: bad record in the table of the best hits");
      std::vector<int32_t> &pp = pairs[(size_t)rec[i].page];
      const int64_t at = (int64_t)pp.size() / 2;
      pp.insert(pp.end(), bp + 2 * x.bp_offset, bp + 2 * (x.bp_offset + x.bp_count));
      x.bp_offset = at;
      x.query -= qa;
      hits[(size_t)rec[i].page].push_back(x);
      if (scored) scores[(size_t)rec[i].page].push_back(job.res.scores[(size_t)i]);
    }
    prb::ScoredView v;
    v.nq = (size_t)(qz - qa + 1);
    v.names = job.names.data() + qa;
    v.qlen_unmasked = job.qlen_unmasked.data() + qa;
    for (size_t p = 0; p < hits.size(); p++)
      v.pages.push_back(PageHits{hits[p].data(), (int64_t)hits[p].size(), pairs[p].data(), (int64_t)pairs[p].size() / 2});
    for (const auto &s : scores) v.scores.push_back(s.data());
    id = scored ? written_or_die(prb::format_scored_batch(v, r.tabs, r.a.o.output_style, id, sink, prb::format_threads())) : write_hits(r, v, id, sink);
    i0 = i1;
  }
  return id;
}

// a table's record names a query of the job and a sequence of the database - and, a group record, a group of the run
bool in_range(const Run &r, size_t nq, const prb_pair_summary &s, int32_t page) {
  return s.query >= 0 && (size_t)s.query < nq && page >= 0 && page < r.npages && s.db_id >= 0 && (size_t)s.db_id < r.tabs[(size_t)page].names.size();
}
bool in_range(const Run &r, size_t nq, const prb_group_pair &x) {
  return in_range(r, nq, x.s, x.page) && x.group >= 0 && (size_t)x.group < r.groups.names.size();
}
// -G: the groups' names and sizes as the formatters take them (`names` keeps the pointers)
template <class View> void set_groups(View &v, const Run &r, std::vector<const char *> &names) {
  for (const std::string &g : r.groups.names) names.push_back(g.c_str());
  v.group_names = names.data();
  v.group_sizes = r.groups.sizes.data();
}

// one job to the output, numbered from `id` on; returns the next id.  The job's handles are freed on return.
int64_t write_job(const Run &r, BatchJob job, int64_t id, LineSink &sink) {
  const int threads = prb::format_threads();
  switch (job.res.mode) {
  case OutputMode::kProfile: {
    prb::ProfileView v;
    set_queries(v, job);
    v.r = prb_profset_rows(job.res.prof.get());
    v.n = prb_profset_size(job.res.prof.get());
    return written_or_die(prb::format_profile_batch(v, r.tabs, id, sink, threads));
  }
  case OutputMode::kScored:
  case OutputMode::kTopHits: return write_tophits(r, job, id, sink);
  case OutputMode::kTop: {
    prb::TopView v;
    set_queries(v, job);
    v.r = prb_topset_pairs(job.res.top.get());
    v.n = prb_topset_size(job.res.top.get());
    return written_or_die(prb::format_top_batch(v, r.tabs, id, sink, threads));
  }
  case OutputMode::kNull: {
    prb::NullView v;
    set_queries(v, job);
    v.r = prb_nullset_pairs(job.res.null.get());
    v.n = prb_nullset_size(job.res.null.get());
    for (int64_t i = 0; i < v.n; i++)
      if (!in_range(r, v.nq, v.r[i].s, v.r[i].page)) die("Error: bad record in the null table");
    if (const prb_null_fdr *f = prb_nullset_fdr(job.res.null.get())) { // (-Q)
      prb::NullFdrView vf;
      static_cast<prb::NullView &>(vf) = v;
      vf.f = f;
      return written_or_die(prb::format_null_fdr_batch(vf, r.tabs, id, sink, threads));
    }
    return written_or_die(prb::format_null_batch(v, r.tabs, id, sink, threads));
  }
  case OutputMode::kGroups: {
    prb::GroupView v;
    set_queries(v, job);
    v.r = prb_groupset_pairs(job.res.groups.get());
    v.n = prb_groupset_size(job.res.groups.get());
    std::vector<const char *> gnames;
    set_groups(v, r, gnames);
    for (int64_t i = 0; i < v.n; i++)
      if (!in_range(r, v.nq, v.r[i])) die("Error: bad record in the group table");
    return written_or_die(prb::format_group_batch(v, r.tabs, id, sink, threads));
  }
  case OutputMode::kFeatures: {
    prb::FeatureView v;
    set_queries(v, job);
    v.r = prb_featset_records(job.res.features.get());
    v.n = prb_featset_size(job.res.features.get());
    std::vector<const char *> fnames;
    for (const std::string &f : r.annot.names) fnames.push_back(f.c_str());
    v.feat_names = fnames.data();
    v.feat_start = r.annot.start.data();
    v.feat_end = r.annot.end.data();
    for (int64_t i = 0; i < v.n; i++)
      if (!in_range(r, v.nq, v.r[i].s, v.r[i].page) || v.r[i].feature < 0 || (size_t)v.r[i].feature >= r.annot.names.size())
        die("Error: bad record in the feature table");
    return written_or_die(prb::format_feature_batch(v, r.tabs, id, sink, threads));
  }
  case OutputMode::kFeatureNull: {
    prb::FNullView v;
    set_queries(v, job);
    v.r = prb_fnullset_records(job.res.fnull.get());
    v.n = prb_fnullset_size(job.res.fnull.get());
    std::vector<const char *> fnames;
    for (const std::string &f : r.annot.names) fnames.push_back(f.c_str());
    v.feat_names = fnames.data();
    v.feat_start = r.annot.start.data();
    v.feat_end = r.annot.end.data();
    for (int64_t i = 0; i < v.n; i++)
      if (!in_range(r, v.nq, v.r[i].f.s, v.r[i].f.page) || v.r[i].f.feature < 0 || (size_t)v.r[i].f.feature >= r.annot.names.size())
        die("Error: bad record in the feature null table");
    return written_or_die(prb::format_fnull_batch(v, r.tabs, id, sink, threads));
  }
  case OutputMode::kGroupNull: {
    prb::GNullView v;
    set_queries(v, job);
    v.r = prb_gnullset_pairs(job.res.gnull.get());
    v.n = prb_gnullset_size(job.res.gnull.get());
    std::vector<const char *> gnames;
    set_groups(v, r, gnames);
    for (int64_t i = 0; i < v.n; i++)
      if (!in_range(r, v.nq, v.r[i].g)) die("Error: bad record in the group null table");
    return written_or_die(prb::format_gnull_batch(v, r.tabs, id, sink, threads));
  }
  case OutputMode::kTargets:
  case OutputMode::kGroupRank:
  case OutputMode::kFeatureRank:
  case OutputMode::kCoverage: return id; // (nothing but progress: the table is written at the end of the run, close_run)
  case OutputMode::kSummary: {
    prb::SummaryView v;
    set_queries(v, job);
    for (const auto &ps : job.res.pair_pages) v.pages.push_back(prb::PagePairs{prb_pairset_pairs(ps.get()), prb_pairset_size(ps.get())});
    return written_or_die(prb::format_summary_batch(v, r.tabs, id, sink, threads));
  }
  case OutputMode::kHits: break;
  }
  BatchView v;
  set_queries(v, job);
  for (const auto &hs : job.res.pages) {
    PageHits ph{prb_hitset_hits(hs.get()), prb_hitset_size(hs.get())};
    ph.bp = prb_hitset_basepairs(hs.get(), &ph.nbp);
    v.pages.push_back(ph);
  }
  return write_hits(r, v, id, sink);
}

// The writer thread turns finished jobs into text in job order while the GPUs already work on the
// next ones (a bounded number of finished jobs wait for it: wait_room).
struct Writer {
  const Run &r;
  std::mutex mu;
  std::condition_variable cv;
  std::map<size_t, BatchJob> done;
  size_t written = 0;
  int64_t total_hits = 0;
  std::thread th;

  explicit Writer(const Run &run) : r(run), th([this] { loop(); }) {}
  void loop() {
    LineSink sink; // text lines go straight to the descriptor (nothing else is written through `out` meanwhile)
    sink.fd = fileno(r.out);
    int64_t id = 0;
    for (size_t b = 0; b < r.njobs && r.rank == 0; b++) {
      BatchJob job;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done.count(b) != 0; });
        job = std::move(done[b]);
        done.erase(b);
      }
      id = write_job(r, std::move(job), id, sink);
      {
        std::lock_guard<std::mutex> lk(mu);
        written = b + 1;
      }
      cv.notify_all();
    }
    total_hits = id;
  }
  // blocks while job `index` is `ahead` jobs or more past the last one written: bounds the results held in memory
  void wait_room(size_t index, size_t ahead) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return index < written + ahead; });
  }
  void submit(size_t index, BatchJob &&job) {
    {
      std::lock_guard<std::mutex> lk(mu);
      done[index] = std::move(job);
    }
    cv.notify_all();
  }
  int64_t join() { // -> the hits written
    th.join();
    return total_hits;
  }
};

// ---- the producers -------------------------------------------------------------------------------
// A worker: its batches one after the other, as next_batch names them; the accessibilities of the next one are computed
// by a helper thread under the worker's second context while this one is searched.  `search` = search_batch, or a team's
// share of it; seed_page: prepare_batch.
using Finish = std::function<void(size_t, const Prepared &, BatchResult &&)>;
using Search = std::function<BatchResult(size_t, Worker &, Prepared &)>;
void run_batches(const Run &r, Worker &w, const std::function<bool(size_t &)> &next_batch, const Finish &finish, const Search &search = {},
                 int seed_page = 0) {
  size_t b = 0, bn = 0;
  bool have = next_batch(b);
  Prepared cur;
  if (have) cur = prepare_batch(r, w.prep_ctx ? w.prep_ctx : w.ctx, w.db, b, seed_page);
  while (have) {
    const bool more = next_batch(bn);
    Prepared nxt;
    std::thread helper;
    std::string helper_error; // (of a team's helper: it ends like its worker)
    bool helper_failed = false;
    if (more && w.prep_ctx)
      helper = std::thread([&, team = t_team_thread] {
        t_team_thread = team;
        try {
          nxt = prepare_batch(r, w.prep_ctx, w.db, bn, seed_page);
        } catch (const TeamError &e) {
          helper_error = e.msg;
          helper_failed = true;
        }
      });
    try {
      finish(b, cur, search ? search(b, w, cur) : search_batch(r, w, cur));
    } catch (...) {
      if (helper.joinable()) helper.join();
      throw;
    }
    if (helper.joinable()) helper.join();
    else if (more) nxt = prepare_batch(r, w.ctx, w.db, bn, seed_page);
    if (helper_failed) die(helper_error);
    cur = std::move(nxt);
    b = bn;
    have = more;
  }
}

// one process: the batches dealt from a counter to the workers, a host thread each
void submit_batch(const Run &r, Writer &writer, size_t b, const Prepared &p, BatchResult &&res) {
  writer.wait_room(b, 2 * r.workers.size() + 1);
  BatchJob job;
  job.res = std::move(res);
  job.qlen_unmasked = p.qlen_unmasked;
  r.names_of(b, job.names);
  writer.submit(b, std::move(job));
}
void worker_main(const Run &r, Worker &w, std::atomic<size_t> &next, Writer &writer) {
  run_batches(
      r, w,
      [&](size_t &b) {
        b = next.fetch_add(1);
        return b < r.nb;
      },
      [&](size_t b, const Prepared &p, BatchResult &&res) { submit_batch(r, writer, b, p, std::move(res)); });
}

// The same with the pages of every batch shared out (PRB_SPLIT): the workers are a team that takes the batches one after
// the other, all of them each batch - everyone with a prb_qbatch of its own, made and given its accessibilities as ever.
// Worker k begins with page k (its seed search started beside the accessibilities), then takes pages from the batch's
// counter until none are left.  A page's hit set or pair set goes into slot p of the batch's one result, whoever searched
// it; in the table modes everyone fills a table of its own, and when all have arrived the first worker merges the others'
// into its own on the device and finishes it.  It hands the result to the writer - one BatchResult per batch, as ever -
// and only then do the others go on (their contexts are not theirs while their tables are merged from).
// A worker that fails raises `failed` with its message and ends; the others end at their next look, the main thread exits.
struct Team {
  struct Batch {
    std::atomic<int> next_page{0};
    BatchResult res;                // what the writer gets: the page slots, or the first worker's table
    std::vector<BatchResult> table; // per worker: its own table (the table modes)
    size_t arrived = 0, left = 0;
    bool taken = false;             // the first worker has merged and handed on
  };
  const Run &r;
  std::mutex mu;
  std::condition_variable cv;
  std::map<size_t, std::shared_ptr<Batch>> batches;
  bool failed = false;
  std::string error;
  std::vector<int64_t> pages_of_worker;

  explicit Team(const Run &run) : r(run), pages_of_worker(run.workers.size(), 0) {}
  std::shared_ptr<Batch> join(size_t b) {
    std::lock_guard<std::mutex> lk(mu);
    std::shared_ptr<Batch> &tb = batches[b];
    if (!tb) {
      tb = std::make_shared<Batch>();
      tb->res = empty_result(r);
      tb->table.resize(r.workers.size());
      tb->next_page = (int)std::min<size_t>(r.workers.size(), (size_t)r.npages);
    }
    return tb;
  }
  void leave(size_t b, Batch &tb) {
    std::lock_guard<std::mutex> lk(mu);
    if (++tb.left == r.workers.size()) batches.erase(b);
  }
  void fail(const std::string &msg) {
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!failed) error = msg;
      failed = true;
    }
    cv.notify_all();
  }
  bool has_failed() {
    std::lock_guard<std::mutex> lk(mu);
    return failed;
  }
  // blocks until `ready` holds (under the lock) - or somebody failed, which ends this worker too
  template <class Ready> void wait(Ready ready) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return failed || ready(); });
    if (failed) throw TeamError{""};
  }
  void signal(const std::function<void()> &change) {
    {
      std::lock_guard<std::mutex> lk(mu);
      change();
    }
    cv.notify_all();
  }

  // worker k's share of batch b; the first worker returns the batch's result, the others an empty one
  BatchResult search(size_t b, size_t k, Worker &w, Prepared &p) {
    const std::shared_ptr<Batch> tb = join(b);
    BatchResult &mine = tb->table[k];
    mine.mode = r.a.mode;
    create_table(r, w, p.qb, mine);
    for (int page = k < (size_t)r.npages ? (int)k : tb->next_page.fetch_add(1); page < r.npages; page = tb->next_page.fetch_add(1)) {
      if (has_failed()) throw TeamError{""};
      search_one_page(r, w, p, page, mine, tb->res);
      pages_of_worker[k]++;
    }
    note_target_queries(r, w, p);
    signal([&] { tb->arrived++; });
    BatchResult res;
    if (k == 0) {
      wait([&] { return tb->arrived == r.workers.size(); });
      std::vector<BatchResult *> others;
      for (size_t j = 1; j < tb->table.size(); j++) others.push_back(&tb->table[j]);
      finish_table(r, w, p, mine, others);
      res = std::move(tb->res);
      res.top = std::move(mine.top);
      res.prof = std::move(mine.prof);
      res.tophits = std::move(mine.tophits);
      res.groups = std::move(mine.groups);
      res.features = std::move(mine.features);
      signal([&] { tb->taken = true; });
    } else {
      wait([&] { return tb->taken; });
      mine = BatchResult(); // (its table, empty by now, freed by its own worker)
    }
    release_batch(p);
    leave(b, *tb);
    return res;
  }
};

void team_main(const Run &r, size_t k, Team &team, Writer &writer) {
  Worker &w = const_cast<Run &>(r).workers[k];
  t_team_thread = true;
  size_t next = 0;
  try {
    run_batches(
        r, w,
        [&](size_t &b) {
          b = next++;
          return b < r.nb;
        },
        [&](size_t b, const Prepared &p, BatchResult &&res) {
          if (k == 0) submit_batch(r, writer, b, p, std::move(res));
        },
        [&](size_t b, Worker &me, Prepared &p) { return team.search(b, k, me, p); }, k < (size_t)r.npages ? (int)k : -1);
  } catch (const TeamError &e) {
    team.fail(e.msg);
  }
}

void run_workers(Run &r, Writer &writer) {
  std::vector<std::thread> threads;
  if (!r.split_pages) {
    std::atomic<size_t> next{0};
    for (Worker &w : r.workers) threads.emplace_back(worker_main, std::cref(r), std::ref(w), std::ref(next), std::ref(writer));
    for (auto &t : threads) t.join();
    return;
  }
  Team team(r);
  for (size_t k = 0; k < r.workers.size(); k++) threads.emplace_back(team_main, std::cref(r), k, std::ref(team), std::ref(writer));
  for (auto &t : threads) t.join();
  if (team.failed) die(team.error);
  if (r.split_given && r.split_knob == kSplitPages) {
    std::string per;
    for (size_t k = 0; k < team.pages_of_worker.size(); k++) per += (k ? "," : "") + std::to_string(team.pages_of_worker[k]);
    std::fprintf(stderr, "page split: %zu batch(es), pages per worker: %s\n", r.nb, per.c_str());
  }
}

// One process per GPU.  The gathers run on a thread of their own, in round order, behind the search of the next batch
// (prb_gather_hits works on the communicator's own stream): rank 0, which receives everybody's records and copies them to
// the host, then takes no longer over a round than the others.  At most two rounds wait for it (their records stay in HBM
// until then).
struct Gatherer {
  struct Round {
    size_t t = 0;
    bool has = false; // this rank has a batch in the round
    std::vector<int32_t> qlen;
    BatchResult res;
  };
  const Run &r;
  Writer &writer;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Round> queue;
  bool closed = false;
  std::thread th;

  Gatherer(const Run &run, Writer &wr) : r(run), writer(wr), th([this] { loop(); }) {}
  void gather(Round &g) {
    BatchJob job;
    for (int page = 0; page < r.npages; page++) {
      prb_hitset *mine = g.res.pages.empty() ? nullptr : g.res.pages[(size_t)page].get(), *all = nullptr;
      if (prb_gather_hits(r.comm, mine, g.has ? (int32_t)g.qlen.size() : 0, g.has ? g.qlen.data() : nullptr, 0, &all))
        die(std::string("Error: ") + prb_last_error());
      if (mine) g.res.pages[(size_t)page].reset();
      if (all) job.res.pages.emplace_back(all);
    }
    if (r.rank != 0) return;
    writer.wait_room(g.t, 3);
    int32_t nr = 0;
    const int32_t *nq_of = nullptr, *ql = nullptr;
    if (!job.res.pages.empty() && prb_hitset_gathered_queries(job.res.pages[0].get(), &nr, &nq_of, &ql)) die(std::string("Error: ") + prb_last_error());
    for (int k = 0; k < nr; k++)
      if (nq_of[k]) r.names_of(g.t * (size_t)r.world + (size_t)k, job.names);
    job.qlen_unmasked.assign(ql, ql + job.names.size());
    writer.submit(g.t, std::move(job));
  }
  void loop() {
    for (;;) {
      Round g;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !queue.empty() || closed; });
        if (queue.empty()) return;
        g = std::move(queue.front());
        queue.pop_front();
      }
      cv.notify_all();
      gather(g);
    }
  }
  // round t: with this rank's batch (p, res), or without one
  void push(size_t t, const Prepared *p, BatchResult &&res) {
    Round g;
    g.t = t;
    g.has = p != nullptr;
    if (p) g.qlen = p->qlen_unmasked;
    g.res = std::move(res);
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return queue.size() < 2; });
    queue.push_back(std::move(g));
    lk.unlock();
    cv.notify_all();
  }
  void close() {
    {
      std::lock_guard<std::mutex> lk(mu);
      closed = true;
    }
    cv.notify_all();
    th.join();
  }
};

// round t: batch t * world + rank; every rank takes part in every round's gather, with or without a batch
void run_ranks(Run &r, Writer &writer) {
  const size_t world = (size_t)r.world, rank = (size_t)r.rank;
  Gatherer gatherer(r, writer);
  size_t t_next = 0;
  run_batches(
      r, r.workers[0],
      [&](size_t &b) {
        b = t_next * world + rank;
        t_next++;
        return b < r.nb;
      },
      [&](size_t b, const Prepared &p, BatchResult &&res) { gatherer.push(b / world, &p, std::move(res)); });
  // rounds in which this rank has no batch left (the last one, when nb is not a multiple of world)
  const size_t mine_rounds = r.nb > rank ? (r.nb - rank + world - 1) / world : 0;
  for (size_t t = mine_rounds; t < r.njobs; t++) gatherer.push(t, nullptr, BatchResult());
  gatherer.close();
}

// -r: the first worker merges the others' tables into its own on the device and finishes it; the lines by page, target
// and rank, numbered from 0
void write_targets(Run &r) {
  Worker &w0 = r.workers[0];
  std::vector<int32_t> qlen(r.seqs.size(), 0);
  for (Worker &w : r.workers) {
    for (const auto &[id, len] : w.target_qlen) qlen[(size_t)id] = len;
    if (&w != &w0 && prb_targetset_merge(w0.ctx, w0.targets, w.targets)) die(prb_last_error());
  }
  if (prb_targetset_finish(w0.ctx, w0.targets)) die(prb_last_error());
  prb::TargetView v;
  v.nq = r.names.size();
  v.names = r.names.data();
  v.qlen_unmasked = qlen.data();
  v.r = prb_targetset_pairs(w0.targets);
  v.n = prb_targetset_size(w0.targets);
  for (int64_t i = 0; i < v.n; i++)
    if (v.r[i].s.query < 0 || (size_t)v.r[i].s.query >= v.nq || v.r[i].page < 0 || v.r[i].page >= r.npages)
      die("Error: bad record in the table of the best queries per target");
  LineSink sink;
  sink.fd = fileno(r.out);
  written_or_die(prb::format_target_batch(v, r.tabs, 0, sink, prb::format_threads()));
}

// -c: the first worker merges the others' tables into its own on the device and reduces it to the regions of depth D;
// the lines by page, target and start, numbered from 0
void write_regions(Run &r) {
  Worker &w0 = r.workers[0];
  std::vector<int32_t> qlen(r.seqs.size(), 0);
  for (Worker &w : r.workers) {
    for (const auto &[id, len] : w.target_qlen) qlen[(size_t)id] = len;
    if (&w != &w0 && prb_covset_merge(w0.ctx, w0.coverage, w.coverage)) die(prb_last_error());
  }
  if (prb_covset_finish(w0.ctx, w0.coverage, r.a.depth)) die(prb_last_error());
  prb::RegionView v;
  v.nq = r.names.size();
  v.names = r.names.data();
  v.qlen_unmasked = qlen.data();
  v.r = prb_covset_regions(w0.coverage);
  v.n = prb_covset_size(w0.coverage);
  for (int64_t i = 0; i < v.n; i++)
    if (v.r[i].query < 0 || (size_t)v.r[i].query >= v.nq || v.r[i].page < 0 || v.r[i].page >= r.npages || v.r[i].db_id < 0 ||
        (size_t)v.r[i].db_id >= r.tabs[(size_t)v.r[i].page].names.size())
      die("Error: bad record in the table of the targets' regions");
  LineSink sink;
  sink.fd = fileno(r.out);
  written_or_die(prb::format_region_batch(v, r.tabs, 0, sink, prb::format_threads()));
}

// -R: the first worker merges the others' tables into its own on the device and finishes it; the lines by group and rank,
// numbered from 0
void write_grouprank(Run &r) {
  Worker &w0 = r.workers[0];
  std::vector<int32_t> qlen(r.seqs.size(), 0);
  for (Worker &w : r.workers) {
    for (const auto &[id, len] : w.target_qlen) qlen[(size_t)id] = len;
    if (&w != &w0 && prb_grouprank_merge(w0.ctx, w0.grouprank, w.grouprank)) die(prb_last_error());
  }
  if (prb_grouprank_finish(w0.ctx, w0.grouprank)) die(prb_last_error());
  prb::GroupView v;
  v.nq = r.names.size();
  v.names = r.names.data();
  v.qlen_unmasked = qlen.data();
  v.r = prb_grouprank_pairs(w0.grouprank);
  v.n = prb_grouprank_size(w0.grouprank);
  std::vector<const char *> gnames;
  set_groups(v, r, gnames);
  for (int64_t i = 0; i < v.n; i++)
    if (!in_range(r, v.nq, v.r[i])) die("Error: bad record in the table of the best queries per group");
  LineSink sink;
  sink.fd = fileno(r.out);
  written_or_die(prb::format_grouprank_batch(v, r.tabs, 0, sink, prb::format_threads()));
}

// -B: the first worker merges the others' tables into its own on the device and finishes it; the lines by feature and
// rank, numbered from 0
void write_featrank(Run &r) {
  Worker &w0 = r.workers[0];
  std::vector<int32_t> qlen(r.seqs.size(), 0);
  for (Worker &w : r.workers) {
    for (const auto &[id, len] : w.target_qlen) qlen[(size_t)id] = len;
    if (&w != &w0 && prb_featrank_merge(w0.ctx, w0.featrank, w.featrank)) die(prb_last_error());
  }
  if (prb_featrank_finish(w0.ctx, w0.featrank)) die(prb_last_error());
  prb::FeatRankView v;
  v.nq = r.names.size();
  v.names = r.names.data();
  v.qlen_unmasked = qlen.data();
  v.r = prb_featrank_records(w0.featrank);
  v.n = prb_featrank_size(w0.featrank);
  std::vector<const char *> fnames;
  for (const std::string &f : r.annot.names) fnames.push_back(f.c_str());
  v.feat_names = fnames.data();
  v.feat_start = r.annot.start.data();
  v.feat_end = r.annot.end.data();
  for (int64_t i = 0; i < v.n; i++)
    if (!in_range(r, v.nq, v.r[i].f.s, v.r[i].f.page) || v.r[i].f.feature < 0 || (size_t)v.r[i].f.feature >= r.annot.names.size())
      die("Error: bad record in the table of the best queries per feature");
  LineSink sink;
  sink.fd = fileno(r.out);
  written_or_die(prb::format_featrank_batch(v, r.tabs, 0, sink, prb::format_threads()));
}

void close_run(Run &r, int64_t total_hits) {
  if (r.a.mode == OutputMode::kTargets && r.rank == 0) write_targets(r);
  if (r.a.mode == OutputMode::kGroupRank && r.rank == 0) write_grouprank(r);
  if (r.a.mode == OutputMode::kFeatureRank && r.rank == 0) write_featrank(r);
  if (r.a.mode == OutputMode::kCoverage && r.rank == 0) write_regions(r);
  if (r.a.binary()) {
    put<int64_t>(r.out, kEnd);
    put<int64_t>(r.out, total_hits);
  }
  if (std::fclose(r.out)) die("Error: can't write the output file");
  if (r.comm) prb_comm_destroy(r.comm);
  for (auto &w : r.workers) {
    prb_targetset_free(w.targets);
    prb_covset_free(w.coverage);
    prb_grouprank_free(w.grouprank);
    prb_featrank_free(w.featrank);
    prb_annot_free(w.annot);
    prb_db_close(w.db);
    if (w.prep_ctx) prb_ctx_destroy(w.prep_ctx);
    prb_ctx_destroy(w.ctx);
  }
}

int ris_main(int argc, char **argv) {
  Run r;
  r.a = parse_args(argc, argv);
  const std::string err = prb::read_fasta(r.a.in, r.names, r.seqs);
  if (!err.empty()) die(err);
  load_pairlist(r);
  load_groups(r);
  load_features(r);
  const std::vector<int> devices = rank_setup(r);
  split_setup(r);
  open_workers(r, devices);
  if (r.rank_mode) r.comm = join_ranks(r);
  read_seq_tables(r);
  open_output(r);
  plan_batches(r);
  plan_split(r);
  Writer writer(r);
  if (r.rank_mode) run_ranks(r, writer);
  else run_workers(r, writer);
  close_run(r, writer.join());
  return 0;
}

// `db` sub-command (db_construction_parameters.cpp getopt string "i:o:r:s:w:d:c:a:p:",
// defaults db_construction_parameters.hpp:41-52): same files as the reference writes.
int db_main(int argc, char **argv) {
  std::string in, out;
  int repeat = 0, hash = 8, W = 70, delta = 5, chunk = 2147483647;
  int c;
  while ((c = getopt(argc, argv, "i:o:r:s:w:d:c:a:p:")) != -1) {
    switch (c) {
    case 'i': in = optarg; break;
    case 'o': out = optarg; break;
    case 'r': repeat = std::atoi(optarg); break;
    case 's': hash = std::atoi(optarg); break;
    case 'w': W = std::atoi(optarg); break;
    case 'd': delta = std::atoi(optarg); break;
    case 'c': chunk = std::atoi(optarg); break;
    case 'a': case 'p': break;
    default: die("Error: invalid argument");
    }
  }
  if (out.empty()) die("Error: -o option is required");
  if (delta <= 1) die("Error: -d option must be greater than 1");
  if (repeat < 0 || repeat > 2) die("Error: -r option must be 0, 1, or 2");
  std::vector<std::string> names, seqs;
  std::string err = prb::read_fasta(in, names, seqs);
  if (!err.empty()) die(err);
  std::string cat;
  std::vector<int64_t> off(seqs.size() + 1, 0);
  std::vector<const char *> np;
  for (size_t i = 0; i < seqs.size(); i++) {
    cat += seqs[i];
    off[i + 1] = (int64_t)cat.size();
    np.push_back(names[i].c_str());
  }
  prb_ctx *ctx = nullptr;
  const char *env = std::getenv("PRB_DEVICES");
  if (prb_ctx_create(env ? std::atoi(env) : 0, nullptr, &ctx)) die(std::string("Error: ") + prb_last_error());
  if (prb_db_build(ctx, out.c_str(), (int32_t)seqs.size(), np.data(), cat.data(), off.data(), repeat, hash, W, delta, chunk))
    die(std::string("Error: ") + prb_last_error());
  prb_ctx_destroy(ctx);
  return 0;
}

} // namespace

int main(int argc, char **argv) {
  if (argc == 1 || std::strcmp(argv[1], "-h") == 0) {
    usage();
    return 0;
  }
  if (std::strcmp(argv[1], "ris") == 0) return ris_main(argc - 1, argv + 1);
  if (std::strcmp(argv[1], "db") == 0) return db_main(argc - 1, argv + 1);
  if (std::strcmp(argv[1], "txt") == 0) return txt_main(argc - 1, argv + 1);
  std::puts("usage: pRIblast-hip [-h] {db | ris | txt} options");
  return 0;
}
