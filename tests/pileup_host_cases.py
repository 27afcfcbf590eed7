"""Helpers of the tests of the pileup on the host-buffer path (docs/GACT_SPEC.md, "Pileup on the host-buffer path and across
replicas"): the ragged batches of the planted workload, the host rule over what a batch returned, the rows that put events on
the first and the last word of every plane, the files of the accaln flow, constructed site and allele tables.  No GPU is
touched at import."""
import ctypes as C

import numpy as np

import pileup_cases as PC
from longreadmapper_amd import capi
from longreadmapper_amd.capi import lib

GUARD = 0xC5C5C5C5
INS_COLS = 8
CUTS = [0, 500, 1111, 1600]                # three ragged batches of the 1600 planted reads
PIPE = dict(sub_batches=3, group_subs=1)   # every batch: three seed sub-batches, three extension groups, two streams
SLICE_READS = 200                          # ... and with this, three to four slices over the slots
MERGE_CHUNK_BYTES = 16 << 20               # the staging buffer of a merge from another device (LRM_PILEUP_MERGE_CHUNK words)


def batches(w, cuts=CUTS):
    """-> [(reads, lens)] fresh copies of the planted reads cut at `cuts` (map_batch modifies reads in place)"""
    return [(w["reads"][a:b].copy(), w["lens"][a:b].copy()) for a, b in zip(cuts, cuts[1:])]


def revcomp(seq):
    return bytes(seq)[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def host_planes(runs, lo, hi, ins_cols, turned=True, min_mapq=None):
    """lrm_pileup_add_host / lrm_pileup_ins_add_host over what batches returned: runs = [(reads as the call left them, lens,
    res)].  turned=False: the caller kept its reads (keep_reads) -- a mapped reverse-strand read is reverse-complemented here.
    min_mapq: only the reads whose res["mapq"] record says at least that.  -> (8 W + 1 words, 4 K W words)"""
    W = hi - lo
    planes, ins = np.zeros(8 * W + 1, dtype=np.uint32), np.zeros(max(4 * ins_cols * W, 1), dtype=np.uint32)
    for reads, lens, res in runs:
        for i in range(len(lens)):
            n_ops = int(res["n_ops"][i])
            if int(res["meta_r"][i]) == 0 or int(res["score"][i]) == -1 or n_ops <= 0:
                continue
            if min_mapq is not None and int(res["mapq"]["mapq"][i]) < min_mapq:
                continue
            read = bytes(reads[i, :lens[i]])
            if not turned and int(res["meta"]["strand"][i]) == 1:
                read = revcomp(read)
            ops = bytes(res["ops"][i, :n_ops])
            loc = int(res["meta"]["loc"][i])
            lib.lrm_pileup_add_host(ops, n_ops, read, len(read), loc, lo, hi, planes.ctypes.data)
            if ins_cols:
                lib.lrm_pileup_ins_add_host(ops, n_ops, read, len(read), loc, lo, hi, ins_cols, ins.ctypes.data)
    return planes, ins[:4 * ins_cols * W]


def dm_raw(dm):
    """the two allocations of a DeviceMapper's accumulator, guard words included (lrm_debug_pileup_raw / _ins_raw)"""
    W = dm.pileup_window[1] - dm.pileup_window[0]
    raw = np.zeros(8 * W + 1 + 16, dtype=np.uint32)
    capi.check(lib.lrm_debug_pileup_raw(dm.pileup, raw.ctypes.data, len(raw), dm._stream()), "lrm_debug_pileup_raw")
    ins = np.zeros(4 * dm.pileup_ins_cols * W + 16, dtype=np.uint32)
    if dm.pileup_ins_cols:
        capi.check(lib.lrm_debug_pileup_ins_raw(dm.pileup, ins.ctypes.data, len(ins), dm._stream()), "lrm_debug_pileup_ins_raw")
    return raw, ins


def guarded(raw):
    """the counter words of a raw dump, after checking the 16 guard words behind them"""
    assert len(raw) > 16 and (raw[-16:] == GUARD).all(), raw[-16:]
    return raw[:-16]


# ---------------------------------------------------------------------------------------------------------
# the merge: rows whose events sit on the first and on the last word of planes
# ---------------------------------------------------------------------------------------------------------
MERGE_WIDTHS = [1, 2, 3, 5, 255, 256, 257, capi.PILEUP_TILE, capi.PILEUP_TILE + 1]
MERGE_KS = [0, 1, 8]


def _row(name, ops, read, loc):
    return PC.Case(name, ops, read, loc, 5, 1, 60, None, False, None)


def edge_rows(lo, W, seed):
    """Rows over the window [lo, lo + W).  `first`: an 'X' on position lo whose read byte is A and a run of nine inserted A's
    behind it -- word 0 of the difference plane, of the x_a and the n_ins plane and of insertion plane (0, A), the first word
    of the second allocation.  `last`: the same on position lo + W - 1 with T's -- the last word of the n_ins plane, which is
    the last word of the first allocation, and of insertion plane (K - 1, T), the last word of the second; its -1 of the depth
    lies in word W of the difference plane.  From 255 positions on a few random rows in between."""
    rows = [_row("first", b"X" + b"I" * 9, b"A" * 10, lo), _row("last", b"X" + b"I" * 9, b"T" * 10, lo + W - 1)]
    if W >= 255:
        rng = np.random.default_rng(seed)
        for k in range(6):
            ops = bytes(rng.choice(np.frombuffer(b"====XIDS", dtype=np.uint8), size=int(rng.integers(20, 200))))
            read = bytes(rng.choice(np.frombuffer(b"ACGTn", dtype=np.uint8), size=max(PC.qlen(ops), 1)))
            rows.append(_row("random-%d" % k, ops, read, lo + int(rng.integers(0, W))))
    return rows


def edge_words(W, K):
    """indices that edge_rows must have made nonzero: (in the first allocation, in the second)"""
    n_ins_plane = W + 1 + 6 * W
    return [0, W, W + 1, n_ins_plane, n_ins_plane + W - 1], ([0, 4 * K * W - 1] if K else [])


# ---------------------------------------------------------------------------------------------------------
# the flow's files; constructed site tables
# ---------------------------------------------------------------------------------------------------------
def write_fasta(path, named_seqs):
    with open(path, "wb") as f:
        for name, s in named_seqs:
            f.write(b">" + name + b"\n")
            b = bytes(s)
            for i in range(0, len(b), 60):
                f.write(b[i:i + 60] + b"\n")


def write_fastq(path, reads, lens):
    with open(path, "wb") as f:
        for i in range(len(lens)):
            s = bytes(reads[i, :lens[i]])
            f.write(b"@read%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n")


def site_tables(mta):
    """Sites on the first and the last base of every sequence of mta [(name, offset, seq_len)] and between them, with alleles
    of 0, 1 and 8 bases (and of 3) -> (PILEUP_SITE_DT records in ascending position, PILEUP_INS_ALLELE_DT records)"""
    pos = []
    for _, off, n in mta:
        pos += sorted({off, off + 1, off + n // 2, off + n - 1})
    sites = np.zeros(len(pos), dtype=capi.PILEUP_SITE_DT)
    alleles = np.zeros(len(pos), dtype=capi.PILEUP_INS_ALLELE_DT)
    lens = [0, 1, 8, 3]
    for k, p in enumerate(pos):
        sites[k] = (p, 40 + k, 30 - k, 5 + k, k % 3, 2 * k, ord("ACGTn"[k % 5]), ord("TGCA."[k % 5]), ord("ACGT-N"[k % 6]), 1 + k % 7)
        ln = lens[k % 4]
        alleles["n_col0"][k], alleles["len"][k], alleles["flags"][k] = 7 * k, ln, k % 4
        alleles["bases"][k, :ln] = np.frombuffer(b"GATTACAT"[:ln], dtype=np.uint8)
    return sites, alleles


def sites_format_ins(host, sites, alleles, room=None):
    """lrm_pileup_sites_format_ins -> (return code, the text)"""
    longest = max(int(host.h.mta[s].name_len) for s in range(host.mta_len))
    room = (longest + 128) * len(sites) + 1 if room is None else room
    buf = C.create_string_buffer(max(room, 1))
    k = lib.lrm_pileup_sites_format_ins(host.h.mta, host.mta_len, sites.ctypes.data if len(sites) else None,
                                        None if alleles is None else alleles.ctypes.data, len(sites), buf, room)
    return k, (buf.raw[:k] if k >= 0 else None)
