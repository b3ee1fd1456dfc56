"""The run-time knob table of INTEGRATION.md (section 5) against the library's source.

Every NMC_* environment variable that csrc/ reads -- a string literal handed to getenv or to
the helpers of ctx.h (nmc_env_int, nmc_env_flag; nmc_env_persist reads NMC_PERSIST through
getenv) -- has a row in the table, and the table has no row for a name the code does not read.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc-for-nested-data_amd", "csrc")

READ = re.compile(r'\b(?:getenv|nmc_env_int|nmc_env_flag)\s*\(\s*"(NMC_[A-Z0-9_]+)"')
ROW = re.compile(r"^\|\s*`(NMC_[A-Z0-9_]+)`\s*\|([^|]*)\|([^|]*)\|([^|]*)\|\s*$")


def knobs_read():
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")):
        with open(path) as f:
            names.update(READ.findall(f.read()))
    return names


def table_rows():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = text.split("## 5. Run-time switches", 1)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.splitlines():
        m = ROW.match(line)
        if m:
            assert m.group(1) not in rows, "two rows for " + m.group(1)
            rows[m.group(1)] = [c.strip() for c in m.groups()[1:]]
    return rows


def test_every_knob_read_has_a_row():
    read, rows = knobs_read(), table_rows()
    assert len(read) >= 30, sorted(read)   # (the scan found the library's knobs at all)
    assert sorted(read - set(rows)) == []


def test_table_names_no_knob_the_code_does_not_read():
    assert sorted(set(table_rows()) - knobs_read()) == []


def test_rows_give_default_kind_and_effect():
    for name, (default, kind, effect) in table_rows().items():
        assert default and effect, name
        assert kind in ("switch", "tuning", "diag", "debug"), (name, kind)


def test_debug_rows_are_the_knobs_behind_nmc_debug_knobs():
    """A name read only between #ifdef NMC_DEBUG_KNOBS and its #endif is marked debug, and
    no other row is."""
    guarded, plain = set(), set()
    for path in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")):
        inside = False
        with open(path) as f:
            for line in f:
                if re.match(r"\s*#\s*ifdef\s+NMC_DEBUG_KNOBS", line):
                    inside = True
                elif inside and re.match(r"\s*#\s*endif", line):
                    inside = False
                else:
                    (guarded if inside else plain).update(READ.findall(line))
    debug = {n for n, (_, kind, _) in table_rows().items() if kind == "debug"}
    assert debug == guarded - plain
