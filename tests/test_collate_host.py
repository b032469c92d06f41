"""CPU: collating alignments by read — the host definition (metalign_amd/collate.py) on a hand table and on generated files, and
the device's key function and record classes (metalign_amd/csrc/mg_collate_core.h) compiled for the host
(tests/host_collate_check.cpp) against an independent MurmurHash3 (tests/indep_sketch.py).  No GPU needed."""
import os
import struct
import subprocess

import pytest

import collate_cases as cc
import indep_sketch
from metalign_amd import cli, collate

HERE = os.path.dirname(os.path.abspath(__file__))


def L(q, flag, cigar="10M", rname="A.1", pos=1):
    return "%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\tNM:i:0\n" % (q, flag, rname, pos, cigar)


def test_hand_table():
    hd, sq = "@HD\tVN:1.6\tSO:coordinate\n", "@SQ\tSN:A.1\tLN:100\n"
    lines = [
        hd,
        L("u", 4, "*"),          # 1  an unmapped-only name: dropped
        L("g", 0, "*"),          # 2  the first line of g is not retained (CIGAR '*'): g's place is its line 9
        L("p", 147),             # 3  mate 2 before mate 1
        L("s", 256),             # 4  a secondary before its primary
        L("w", 193),             # 5  flag 64 | 128: not the mate-2 class
        sq,                      # 6  a header line in the middle: kept, in front
        L("p", 99),              # 7
        L("s", 0),               # 8
        L("g", 16),              # 9
        L("w", 129),             # 10 mate 2
        L("s", 2048),            # 11 a supplementary: after the primary, file order among the not-primary
        L("p", 355),             # 12 mate 1's secondary: before every mate-2 line
        L("p", 403),             # 13 mate 2's secondary
        "short\t0\tA.1\n",       # 14 fewer than 6 fields: dropped
        L("g", 256),             # 15
    ]
    want = [lines[i] for i in (0, 6,
                               7, 12, 3, 13,   # p: 99, 355 | 147, 403
                               8, 4, 11,       # s: 0 | 256, 2048 (file order)
                               5, 10,          # w: 193 | 129
                               9, 15)]         # g
    assert collate.collated_lines(lines) == want
    assert collate.collated_lines([ln.encode() for ln in lines]) == [ln.encode() for ln in want]  # (bytes lines, as files give them)
    assert collate.collated_lines(want) == want  # a fixed point
    assert collate.collated_lines([]) == []
    assert collate.collated_lines([hd, sq]) == [hd, sq]
    one = [L("x", 256), L("x", 0), L("x", 2048)]
    assert collate.collated_lines(one) == [one[1], one[0], one[2]]  # one group only
    distinct = [L("n%d" % i, 16 * (i & 1)) for i in range(7)]
    assert collate.collated_lines(distinct) == distinct  # all names distinct
    assert collate.collated_lines([L("u", 4, "*"), L("u", 77, "*")]) == []
    assert collate.header_says_coordinate([hd, sq]) and not collate.header_says_coordinate([hd.replace("coordinate", "unsorted"), sq])
    with pytest.raises(ValueError):
        collate.collated_lines(["x\tnotanumber\tA.1\t1\t60\t10M\n"])  # int(FLAG), as the reference


def test_name_grouped_output_is_a_fixed_point_and_a_shuffle_is_not():
    _, accs, acc_index, text = cc.case(300, 100)
    lines = text.splitlines(True)
    got = collate.collated_lines(lines)
    kept = [ln for ln in lines if ln.startswith("@")] + [ln for ln in lines if not ln.startswith("@") and collate._retained(ln)]
    assert got == kept and len(got) > 400
    shuffled = cc.coordinate_shuffle(text)
    back = collate.collated_lines(shuffled)
    assert back != [ln for ln in shuffled if ln.startswith("@") or collate._retained(ln)]  # it changes something
    assert sorted(back) == sorted(ln for ln in shuffled if ln.startswith("@") or collate._retained(ln))
    names = [ln.split("\t")[0] for ln in back if not ln.startswith("@")]
    runs = [n for i, n in enumerate(names) if i == 0 or names[i - 1] != n]
    assert len(runs) == len(set(names))  # every read is ONE run now


def test_the_option_is_an_optional_flag_with_three_values():
    for tool in ("map_and_profile", "metalign"):
        p = cli.parser_for(tool)
        act = [a for a in p._actions if a.dest == "collate"][0]
        assert act.default == "never" and list(act.choices) == ["never", "auto", "always"] and act.option_strings == ["--collate"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("collate") / "host_collate_check")
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-Wall", "-o", out, os.path.join(HERE, "host_collate_check.cpp")])
    return out


def test_core_header_keys_and_classes(exe, tmp_path):
    names = cc.KEY_NAMES
    assert {len(n) for n in names} >= {1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 254}
    p = tmp_path / "names.bin"
    p.write_bytes(struct.pack("<I", len(names)) + b"".join(struct.pack("<I", len(n)) + n for n in names))
    out = subprocess.run([exe, str(p)], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:]
    lines = out.stdout.decode().splitlines()
    assert lines[0] == "seed %d" % cc.SEED
    keys = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("key ")]
    assert keys == [indep_sketch.murmur3_x64_128(n, cc.SEED) for n in names]
    assert len(set(keys)) == len(set(names))
    classes = [ln for ln in lines if ln.startswith("classes ")][0].split()[1]
    assert [int(c) for c in classes] == [2 * collate.sort_key(f, 0)[0] + collate.sort_key(f, 0)[1] for f in range(4096)]
