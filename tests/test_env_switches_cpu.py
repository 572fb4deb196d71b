"""The environment switches of libaclgpu.so: INTEGRATION.md's table lists exactly the ACL_* variables the C++ sources read, the
switches deleted with their A/B's losing side stay deleted, and every switch a test sets is a listed one.  Reads files only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spicedb-kubeapi-proxy_amd")
CSRC = os.path.join(PKG, "csrc")

# settled A/B switches, deleted with the paths only they reached (the measurements stay under profiles/)
DELETED = ["ACL_LOCAL_UPW", "ACL_LOCAL_STATIC_PCT", "ACL_LOCAL_DYN_UNIT", "ACL_LOCAL_BLOCKS_WIDE", "ACL_LOCAL_WIDE_MIN", "ACL_HOSTMAP_MAX",
           "ACL_HOST_SKEW_PCT", "ACL_REV_ROWS", "ACL_KEEP_RESOLVE", "ACL_INTERN_REPEAT", "ACL_INTERN_PIN", "ACL_SLOT_HUGE_PAGES"]
# variables that bench.py and the tests define for themselves: the library never reads them
OWN = ["ACL_ROOT", "ACL_SKIP_C5_FULL", "ACL_EXCHANGE"]
OWN_PREFIXES = ["ACL_BENCH_"]


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _files(top, skip=()):
    for d, dirs, names in os.walk(top):
        dirs[:] = [x for x in dirs if os.path.join(d, x) not in skip and x != "__pycache__"]
        for nm in names:
            if not nm.endswith((".pyc", ".so", ".o")):
                yield os.path.join(d, nm)


def _table():
    """{name: (default, read, class)} of the section "Environment switches" of INTEGRATION.md"""
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    m = re.search(r"^#+ Environment switches\n(.*?)(?=^#+ )", text, re.M | re.S)
    assert m, "INTEGRATION.md has no section 'Environment switches'"
    rows = {}
    for line in m.group(1).splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if len(cells) == 4 and re.fullmatch(r"`ACL_[A-Z0-9_]+`", cells[0]):
            name = cells[0].strip("`")
            assert name not in rows, f"{name} is listed twice"
            rows[name] = tuple(cells[1:])
    return rows


def test_table_lists_what_the_sources_read():
    # a name reaches getenv as a string literal: directly, or through the batcher's knob(name, default) -- so every quoted ACL_* name counts
    read, direct = set(), set()
    for path in _files(CSRC):
        text = _read(path)
        read |= set(re.findall(r'"(ACL_[A-Z0-9_]+)"', text))
        direct |= set(re.findall(r'getenv\(\s*"(ACL_[A-Z0-9_]+)"', text))
    assert direct and direct <= read
    table = _table()
    assert set(table) == read, f"not in the table: {sorted(read - set(table))}; in the table but never read: {sorted(set(table) - read)}"
    for name, (default, when, cls) in table.items():
        assert default and when, name
        assert cls in ("operator", "test", "debug"), (name, cls)


def test_deleted_switches_stay_deleted():
    tools = os.path.join(ROOT, "tools")
    paths = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "README.md"), os.path.join(ROOT, "INTEGRATION.md")]
    paths += list(_files(CSRC)) + list(_files(os.path.join(PKG, "aclgpu"))) + list(_files(os.path.join(ROOT, "tests")))
    paths += list(_files(tools, skip=(os.path.join(tools, "runs"), os.path.join(tools, "bin"))))
    gone = re.compile(r"\b(" + "|".join(DELETED) + r")\b")
    found = []
    for path in paths:
        if os.path.abspath(path) == os.path.abspath(__file__):  # (this list)
            continue
        found += [(os.path.relpath(path, ROOT), nm) for nm in sorted(set(gone.findall(_read(path))))]
    assert not found, found


def test_switches_the_tests_set_are_listed():
    table = _table()
    sets = [re.compile(r'setenv\(\s*["\'](ACL_[A-Z0-9_]+)["\']'), re.compile(r'environ\[\s*["\'](ACL_[A-Z0-9_]+)["\']\s*\]\s*=[^=]'),
            re.compile(r'\b(ACL_[A-Z0-9_]+)=[^=]')]  # (the last: dict(os.environ, ACL_X="..."), the environment of a child process)
    unlisted = []
    for path in _files(os.path.join(ROOT, "tests")):
        if not path.endswith(".py") or os.path.abspath(path) == os.path.abspath(__file__):
            continue
        text = _read(path)
        for rx in sets:
            for nm in rx.findall(text):
                if nm in OWN or any(nm.startswith(p) for p in OWN_PREFIXES) or nm in table:
                    continue
                unlisted.append((os.path.relpath(path, ROOT), nm))
    assert not unlisted, unlisted
