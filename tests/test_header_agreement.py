"""The Python copies of the ABI (longreadmapper_amd/records.py) against include/*.h themselves: a C program generated from
the Python tables prints sizeof / offsetof of every member of every bound struct and every mirrored #define; the host C
compiler is the judge.  A member the header does not have fails to compile, one the table lacks changes a size or an offset."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from longreadmapper_amd import capi, mapper, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def members(s):
    return records.MAP_OPTION_FIELDS if s is records.MapOptions else [f[0] for f in s._fields_]


DTYPES = {records.Entry: "ENTRY_DT", records.SeqMeta: "META_DT", records.Anchor: "ANCHOR_DT", records.Clip: "CLIP_DT",
          records.Segment: "SEGMENT_DT", records.Mapq: "MAPQ_DT", records.AlnSummary: "SUMMARY_DT", records.Cigar: "CIGAR_DT"}


@pytest.fixture(scope="module")
def header_says(tmp_path_factory):
    """{"sizeof T": n, "T.member": offset, "LRM_X": value} as the compiled headers have them."""
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "lrm_accel.h"', '#include "lrm_index_host.h"',
             '#include "lrm_io_host.h"', 'int main(void) {']
    for s, c_name in records.STRUCTS.items():
        lines.append('    printf("sizeof %s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        lines += ['    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c_name, f, c_name, f) for f in members(s)]
    lines += ['    printf("%s %%lld\\n", (long long) (%s));' % (name, name) for name in records.CONSTANTS]
    lines += ['    return 0;', '}']
    d = tmp_path_factory.mktemp("header_agreement")
    src, exe = d / "layout.c", d / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True)
    return {key: int(value) for key, value in (line.rsplit(" ", 1) for line in out.splitlines())}


def test_every_struct_has_the_headers_size_and_offsets(header_says):
    assert len(records.STRUCTS) == 25 == len(set(records.STRUCTS.values()))
    bound = {v for v in vars(capi).values() if isinstance(v, type) and issubclass(v, C.Structure) and not v.__name__.startswith("_")}
    assert bound == set(records.STRUCTS)                         # no struct of the binding escapes the comparison
    for s, c_name in records.STRUCTS.items():
        assert C.sizeof(s) == header_says["sizeof " + c_name], c_name
        covered = 0
        for f in members(s):
            member = getattr(s, f)
            assert member.offset == header_says["%s.%s" % (c_name, f)], (c_name, f)
            covered = max(covered, member.offset + member.size)
        assert C.sizeof(s) - covered < C.alignment(s), c_name   # nothing but tail padding behind the last member


def test_every_record_dtype_has_the_headers_offsets(header_says):
    for s, name in DTYPES.items():
        dt = getattr(records, name)
        c_name = records.STRUCTS[s]
        assert getattr(mapper, name) is dt and dt.itemsize == header_says["sizeof " + c_name], name
        c_names = {"_pad" if f == "pad" else f: f for f in members(s)}
        named = [f for f in dt.names if f in c_names]
        assert len(named) == len(c_names), name
        for f in named:
            sub, off = dt.fields[f][:2]
            assert off == header_says["%s.%s" % (c_name, c_names[f])] and sub.itemsize == getattr(s, c_names[f]).size, (name, f)
        rest = [f for f in dt.names if f not in c_names]             # only the tail padding may come on top, as opaque bytes
        assert rest in ([], ["_pad"]) and all(dt.fields[f][0].kind == "V" and dt.fields[f][1] >= max(dt.fields[g][1] for g in named)
                                              for f in rest), name
    assert np.zeros(1, records.META_DT)["_pad"].dtype == np.dtype("V3")


def test_every_mirrored_constant_has_the_headers_value(header_says):
    assert len(records.CONSTANTS) >= 14
    for name, value in records.CONSTANTS.items():
        assert header_says[name] == value, name
    assert mapper.N_KERNELS == header_says["LRM_N_KERNELS"] and mapper.DEFAULT_GACT == tuple(
        header_says["LRM_GACT_%s_DEFAULT" % x] for x in "TOW")
