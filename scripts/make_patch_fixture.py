#!/usr/bin/env python3
"""Records what tests/test_integration_patch.py checks integration/oarfish-mi355x.patch against, so that the test needs
no checkout of the reference: per file the patch modifies, the sha256 and line count of the v0.10.3 file, and per hunk
the sha256 of the reference's lines at the hunk's stated position; plus the files the patch creates, which must not
exist there.  Only hashes and names are kept (tests/golden/reference_patch_preimage.json), none of the reference's text.
Run again whenever the patch changes:  python scripts/make_patch_fixture.py <oarfish v0.10.3 checkout>
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_integration_patch import FIXTURE, PATCH, lines_sha256, patch_hunks  # noqa: E402


def main(ref):
    r = subprocess.run(["git", "apply", "--check", PATCH], cwd=ref, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("the patch does not apply to " + ref + ":\n" + r.stderr)
    files, created = {}, []
    for path, old_start, old_lines, _pre in patch_hunks(open(PATCH).read()):
        if old_start == 0 and old_lines == 0:
            assert not os.path.exists(os.path.join(ref, path)), path
            created.append(path)
            continue
        if path not in files:
            data = open(os.path.join(ref, path), "rb").read()
            files[path] = dict(sha256=hashlib.sha256(data).hexdigest(), lines=len(data.decode().splitlines()), hunks=[])
        src = open(os.path.join(ref, path)).read().splitlines()
        files[path]["hunks"].append(dict(old_start=old_start, old_lines=old_lines,
                                         sha256=lines_sha256(src[old_start - 1:old_start - 1 + old_lines])))
    doc = dict(reference="COMBINE-lab/oarfish v0.10.3", files=files, created=created)
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(FIXTURE)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
