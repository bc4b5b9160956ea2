"""The DSRL_* environment switches: every one the package reads has a row in DESIGN.md §9 and the other way round, and every read goes through
one of the two helpers - knob() / knob_str() in csrc/common.h, _lib.knob() in Python."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'dualsuperreslearningforsemseg_amd')


def sources(*exts):
    return sorted(p for e in exts for p in glob.glob(os.path.join(PKG, '**', '*.' + e), recursive=True))


def table():
    """{switch: 'read by' column} of the table in DESIGN.md §9"""
    text = open(os.path.join(ROOT, 'DESIGN.md')).read()
    sec = text.split('\n## 9. Environment switches\n')[1].split('\n## ')[0]
    return {m.group(1): m.group(2).strip() for m in re.finditer(r'^\| `(DSRL_[A-Z0-9_]+)` \|[^|]*\|([^|]*)\|', sec, re.M)}


def reads():
    c, py = set(), set()
    for p in sources('hip', 'h'):
        c.update(re.findall(r'\bknob(?:_str)?\(\s*"(DSRL_[A-Z0-9_]+)"', open(p).read()))
    for p in sources('py'):
        py.update(re.findall(r'\bknob\(\s*[\'"](DSRL_[A-Z0-9_]+)[\'"]', open(p).read()))
    return c, py


def test_every_switch_read_has_a_row_and_every_row_a_read():
    rows = table()
    c, py = reads()
    assert len(rows) >= 40 and c and py
    listed = {n for n, where in rows.items() if where != 'bench'}
    assert c | py == listed, sorted((c | py) ^ listed)
    for n in listed:
        want = ', '.join(w for w, s in (('C', c), ('Python', py)) if n in s)
        assert rows[n] == want, (n, rows[n], want)


def test_switches_are_read_through_the_two_helpers_only():
    for p in sources('hip', 'h'):
        lines = [ln for ln in open(p).read().splitlines() if 'getenv(' in ln]
        if os.path.basename(p) == 'common.h':
            assert len(lines) == 1 and 'knob_str(const char* name)' in lines[0], lines
        else:
            assert not lines, (p, lines)
    for p in sources('py'):
        src = open(p).read()
        assert 'getenv(' not in src, p
        assert not re.search(r'os\.environ\.get\(\s*[\'"]DSRL_|os\.environ\[\s*[\'"]DSRL_', src), p
