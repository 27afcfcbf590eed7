"""Constructed batches for the line fetch of seed_search_kernel behind the presence bitmap, in the form that addresses a
line by a 32-bit offset (seed_kernels.hip: sd_filter_issue32, sd_issue_filtered32, sd_finish_quad32): what the batches of
tests/seed_filter_cases.py do not pin.

One text: 20 kbp of random bases, indexed with its reverse complement (40 kbp), in which one 17-base core -- the bases that
the seeds of four neighbouring read positions share -- stands four times, each time under other three bases to its left
and to its right.  An S-mer enters the seed table once per role r = 0 .. 3 (r bases of it to the right of its core, 3 - r
to the left), so the line of that core is asked to hold sixteen entries: eight find room, the others go to the side table
and the line's overflow mark is set.  The core is chosen so that its line is LINE 0 of the table whatever the number of
lines (line_of below restates sd_key_of's hash): the first line of the table is the one a fetch that needs no particular
line would most naturally name, and a seed that is absent from the text must not be answered from it.

Every batch states a property of its reads against the TEXT alone; tests/test_seed_lines_cases_cpu.py proves each by brute
force (constructed.census), tests/test_gpu_seed_lines.py runs them."""
import numpy as np

import constructed as K
import seed_filter_cases as F

S, P, THRES = F.S, F.P, F.THRES
FWD = 20_000
CORE_LEN = S - 3
# the 34 bits of the core, first base lowest: the low 32 bits times sd_key_of's constant give m = 5, and the two bits above
# them equal m & 3, so the line index is 0 for every table of 2^3 .. 2^31 lines
HASH_MUL = 0x9E3779B1
_M = 5
CORE_CODE = ((_M & 3) << 32) | ((_M * pow(HASH_MUL, -1, 1 << 32)) & 0xFFFFFFFF)
CORE = bytes(b"ACGT"[(CORE_CODE >> (2 * i)) & 3] for i in range(CORE_LEN))
FLANKS = ((b"ACG", b"TGA"), (b"CGT", b"GAC"), (b"GTA", b"ATG"), (b"TAC", b"CCT"))       # (left, right) of the four copies
COPY_AT = (3_001, 7_502, 12_003, 16_504)                                             # first base of the left flank
CROWD_LEN, CROWD_LEAD = 120, 40
# positions with a seed (length - S): 1, 2, 3; 65, 66, 67 (1, 2, 3 mod 4 behind one whole wavefront: the last quad has one,
# two, three seeded lanes, 65 is 1 mod 64: a wavefront with a single live quad); 257 (1 mod 256: a last iteration with one
# seeded lane); 2049 (a second workgroup with one)
RAGGED = tuple(n + S for n in (1, 2, 3, 65, 66, 67, 257, 2049))
BATCHES = ("crowd", "random", "ragged")


def line_of(core_code, bits):
    """sd_key_of's line index of a core of 2 * CORE_LEN = 34 bits in a table of 2^bits lines."""
    m = (core_code & 0xFFFFFFFF) * HASH_MUL & 0xFFFFFFFF
    chi = ((core_code >> 32) ^ m) & 3
    rb = 2 * CORE_LEN - bits
    return (chi << (32 - rb)) | (m >> rb)


def forward():
    """The forward sequence (bytes)."""
    rng = np.random.default_rng(2001)
    a = np.frombuffer(K._filler(rng, FWD), dtype=np.uint8).copy()
    for at, (left, right) in zip(COPY_AT, FLANKS):
        s = left + CORE + right
        a[at:at + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return bytes(a)


def core_pairs(content):
    """Every distinct (role, S-mer) of the text whose core in that role is CORE: the entries its line is asked to hold."""
    text = bytes(content)
    out = set()
    at = text.find(CORE)
    while at >= 0:
        for r in range(4):                       # role r: 3 - r bases of the S-mer lie left of the core
            a = at - (3 - r)
            if a >= 0 and a + S <= len(text) - 1:
                out.add((r, text[a:a + S]))
        at = text.find(CORE, at + 1)
    return out


def batch(name, seq):
    """The reads (list of bytes) of one batch over the forward sequence `seq`."""
    rng = np.random.default_rng(2002 + BATCHES.index(name))
    if name == "crowd":           # clean windows over every copy, the copy at all four positions mod 4 of the read
        return [seq[at - CROWD_LEAD - d:at - CROWD_LEAD - d + CROWD_LEN] for at in COPY_AT for d in range(4)]
    if name == "random":          # independent random sequence: no seed of any read is in the text
        return [K._filler(rng, n) for n in (3_000, 2_048 + S, 257 + S, 65 + S, 66 + S, 67 + S, 1 + S, 5_000)]
    assert name == "ragged"       # clean windows of the text
    return [seq[5_000 + 41 * i:5_000 + 41 * i + n] for i, n in enumerate(RAGGED)]


rows, seed_counts = F.rows, F.seed_counts
