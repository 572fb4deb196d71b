#!/usr/bin/env python3
"""Regenerates tests/golden/bootstrap.json from the reference's embedded
bootstrap file (pkg/spicedb/bootstrap.yaml:1-40).  Run in the build container
only (/root/reference does not exist on the GPU box); the output is committed.

ref_index.json records what tests/test_abi.py needs to know of the reference
checkout, so that the test runs without it: the line count of every .go / .yaml /
.mod file (the citations in this repository must land inside them) and, for each
hunk of shim/patches/options_gpu_scheme.patch, a SHA-256 of the lines the hunk
expects to find (its context and removed lines) at its position in the file.

kats.json is hand-written: each entry restates, as a request/response sequence
at the v1.PermissionsServiceClient seam, an assertion the reference's own tests
make (source file:line in each entry's "source").
"""
import hashlib
import json
import os
import re
import sys

REF = "/root/reference/pkg/spicedb/bootstrap.yaml"
HERE = os.path.dirname(os.path.abspath(__file__))
PATCH = os.path.join(os.path.dirname(os.path.dirname(HERE)), "shim", "patches", "options_gpu_scheme.patch")


def lines_sha256(lines):
    return hashlib.sha256("".join(ln + "\n" for ln in lines).encode()).hexdigest()


def patch_hunks(text):
    """[(file, old start, old lines)] of a unified diff: the lines each hunk expects in the original file."""
    out, path, want = [], None, 0
    for ln in text.split("\n"):
        if want == 0 and ln.startswith("--- a/"):
            path = ln[6:].split("\t")[0]
        elif want == 0 and ln.startswith("@@"):
            m = re.match(r"@@ -(\d+)(?:,(\d+))?", ln)
            want = int(m.group(2) or 1)
            out.append((path, int(m.group(1)), []))
        elif want and ln[:1] in (" ", "-", ""):
            out[-1][2].append(ln[1:])  # (an empty line: a context line whose leading blank an editor dropped)
            want -= 1
    return out


def ref_index(ref_root):
    files = {}
    for dp, dn, fns in os.walk(ref_root):
        dn[:] = sorted(d for d in dn if d != ".git")
        for fn in sorted(fns):
            if fn.rsplit(".", 1)[-1] in ("go", "yaml", "mod"):
                with open(os.path.join(dp, fn), errors="ignore") as fh:
                    files[os.path.relpath(os.path.join(dp, fn), ref_root)] = sum(1 for _ in fh)
    hunks = []
    for path, start, old in patch_hunks(open(PATCH).read()):
        with open(os.path.join(ref_root, path), errors="ignore") as fh:
            have = fh.read().split("\n")[start - 1:start - 1 + len(old)]
        hunks.append({"file": path, "start": start, "lines": len(old), "sha256": lines_sha256(have)})
    return {"source": "the reference checkout: line counts of its .go / .yaml / .mod files; options_gpu_scheme.patch's hunks", "files": files, "patch_hunks": hunks}


def main():
    import yaml

    with open(REF) as f:
        doc = yaml.safe_load(f)
    out = {
        "source": "pkg/spicedb/bootstrap.yaml:1-40",
        "schema": doc["schema"],
        "relationships": [l.strip() for l in doc["relationships"].splitlines() if l.strip()],
    }
    with open(os.path.join(HERE, "bootstrap.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote bootstrap.json:", len(out["schema"]), "schema bytes,", len(out["relationships"]), "relationships")
    idx = ref_index(REF[:REF.index("/pkg/")])
    with open(os.path.join(HERE, "ref_index.json"), "w") as f:
        json.dump(idx, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote ref_index.json:", len(idx["files"]), "files,", len(idx["patch_hunks"]), "patch hunks")


if __name__ == "__main__":
    sys.exit(main())
