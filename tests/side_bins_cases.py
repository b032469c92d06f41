"""Cases for the device building blocks the side outputs share (metalign_amd/csrc/mg_side_dev.h), used by
test_gpu_{coverage,depth,identity,variants}.py.

More accessions than a workgroup's hashed LDS bins have slots: with the family's grid knob at 1 every key goes through ONE table, so
NACC - slots of them cannot get a slot whatever the hash does and add to memory directly.  Every accession gets one to three
records, in an order that mixes the accessions within every wavefront; a few records name rows at or beyond NACC."""
import os
import re

import numpy as np

NACC = 3000
LENGTH = 64
NAMES = ["o%d" % i for i in range(NACC)]
BEYOND = (NACC, NACC + 1, NACC + 77, 0x7FFFFFFF)
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "metalign_amd", "csrc")


def slots(unit, name):
    """The slots of a workgroup's per-accession bins as `unit` (a file of csrc) sets them in the constant `name`."""
    m = re.search(r"\b%s = (\d+)\b" % name, open(os.path.join(CSRC, unit)).read())
    assert m, (unit, name)
    return int(m.group(1))


def rows(seed=11):
    """-> the rows of the records, shuffled: every accession one to three times, each row of BEYOND twice."""
    rng = np.random.default_rng(seed)
    r = np.concatenate([np.repeat(np.arange(NACC), rng.integers(1, 4, NACC)), np.repeat(np.array(BEYOND), 2)])
    rng.shuffle(r)
    assert set(r.tolist()) == set(range(NACC)) | set(BEYOND)
    return [int(x) for x in r]


def overflows(unit, name):
    """The keys that cannot get a slot in one workgroup's table (the case is about them: more than a thousand)."""
    spill = NACC - slots(unit, name)
    assert spill > 1000, "the case needs many more accessions than %s has slots" % name
    return spill
