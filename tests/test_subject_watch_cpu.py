"""Subject-direction watch sets without a GPU: what acl_watch_set_open_subjects refuses, and that the flag and the record are what include/aclgpu.h says."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "aclgpu.h")
SCHEMA = """
definition user {}
definition pod {
  relation viewer: user | user:*
  relation banned: user
  permission view = viewer - banned
}
"""


def open_subjects(aclgpu, e, rt="pod", perm="view", st="user", srel=-1):
    out = C.c_void_p()
    rc = e._L.acl_watch_set_open_subjects(e._h, e.type_id(rt), e.relation_id(rt, perm), e.type_id(st), srel, C.byref(out))
    return rc, out


def test_a_store_only_engine_answers_unavailable(aclgpu_lib):
    import aclgpu
    with aclgpu.Engine(SCHEMA, store_only=True) as e:
        e.touch(("pod", "p0", "viewer", "user", "u0", ""))
        rc, out = open_subjects(aclgpu, e)
        assert rc == aclgpu.ERR_UNAVAILABLE and not out.value and b"store-only" in aclgpu_lib.acl_last_error()
        try:
            e.subject_watch_set("pod", "view", "user")
            raise AssertionError("opened a subject-direction set without a device")
        except aclgpu.AclError as ex:
            assert ex.code == aclgpu.ERR_UNAVAILABLE
        # an unknown permission or subject relation is refused before that, as for acl_watch_set_open
        out = C.c_void_p()
        assert e._L.acl_watch_set_open_subjects(e._h, e.type_id("pod"), 99, e.type_id("user"), -1, C.byref(out)) == aclgpu.ERR_FAILED_PRECONDITION
        assert e._L.acl_watch_set_open_subjects(e._h, e.type_id("pod"), e.relation_id("pod", "view"), e.type_id("user"), 5, C.byref(out)) == aclgpu.ERR_FAILED_PRECONDITION
        rows = np.zeros(4, dtype=np.uint32)
        rid = np.zeros(1, dtype=np.uint32)
        assert e._L.acl_selfcheck_subject_rows(e._h, e.type_id("pod"), e.relation_id("pod", "view"), e.type_id("user"), -1, rid.ctypes.data, 1, rows.ctypes.data,
                                               4) == aclgpu.ERR_UNAVAILABLE


def test_one_of_two_shards_answers_failed_precondition(aclgpu_lib):
    import aclgpu
    with aclgpu.Engine(SCHEMA, store_only=True) as e:
        e._check(e._L.acl_shard_configure(e._h, 0, 2))
        rc, out = open_subjects(aclgpu, e)
        assert rc == aclgpu.ERR_FAILED_PRECONDITION and not out.value and b"shard" in aclgpu_lib.acl_last_error()


def test_null_arguments_answer_invalid_argument(aclgpu_lib):
    import aclgpu
    L = aclgpu_lib
    with aclgpu.Engine(SCHEMA, store_only=True) as e:
        out = C.c_void_p()
        assert L.acl_watch_set_open_subjects(None, 0, 0, 0, -1, C.byref(out)) == aclgpu.ERR_INVALID_ARGUMENT
        assert L.acl_watch_set_open_subjects(e._h, 1, 2, 0, -1, None) == aclgpu.ERR_INVALID_ARGUMENT
        assert L.acl_selfcheck_subject_rows(None, 1, 2, 0, -1, None, 0, None, 0) == aclgpu.ERR_INVALID_ARGUMENT
        assert L.acl_selfcheck_subject_rows(e._h, 1, 2, 0, -1, None, 1, None, 4) == aclgpu.ERR_INVALID_ARGUMENT


def test_the_flag_and_the_record_are_what_the_header_says(aclgpu_lib, tmp_path):
    import aclgpu
    hdr = open(HEADER).read()
    m = re.search(r"#define\s+ACL_WATCH_CHANGE_WILDCARD\s+(\d+)u", hdr)
    assert m and int(m.group(1)) == aclgpu.WATCH_CHANGE_WILDCARD == 1
    src = tmp_path / "rec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aclgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %u\\n", sizeof(acl_watch_change_t), '
                   'offsetof(acl_watch_change_t, watcher), offsetof(acl_watch_change_t, resource_id), offsetof(acl_watch_change_t, gained), '
                   'offsetof(acl_watch_change_t, reserved), ACL_WATCH_CHANGE_WILDCARD); return 0; }\n')
    exe = tmp_path / "rec"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["16", "0", "4", "8", "12", "1"]
    d = aclgpu.WATCH_CHANGE_DTYPE
    assert d.itemsize == 16 and [d.fields[n][1] for n in ("watcher", "resource_id", "gained", "reserved")] == [0, 4, 8, 12]
    assert [f for f, _t in aclgpu._lib.WatchChange._fields_] == ["watcher", "resource_id", "gained", "reserved"] and C.sizeof(aclgpu._lib.WatchChange) == 16
