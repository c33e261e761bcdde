"""integration/oarfish-mi355x.patch: the reference-side binding as a diff against COMBINE-lab/oarfish v0.10.3 -- the
`mi355x` cargo feature, `src/em_gpu.rs` (extern "C" block + shim), the `boundaries()` accessor and the feature-gated
call sites (bulk.rs:155-159, :179, single_cell.rs:150).  No Rust toolchain exists in this image, so the patch is pinned
as far as the image allows: it applies to the reference's v0.10.3 files (pinned by the hashes of
tests/golden/reference_patch_preimage.json), and its extern declarations and #[repr(C)] structs agree with
include/oarfish_em.h name for name, argument count for argument count, field for field."""
import hashlib
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "integration", "oarfish-mi355x.patch")
HEADER = os.path.join(ROOT, "include", "oarfish_em.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_patch_preimage.json")


def lines_sha256(lines):
    return hashlib.sha256("".join(line + "\n" for line in lines).encode()).hexdigest()


def patch_hunks(patch_text):
    """(path, old_start, old_lines, pre-image lines) of every hunk; the line counts of each hunk are checked against
    its header, as `git apply` checks them."""
    out, path, lines = [], None, patch_text.splitlines()
    i = 0
    while i < len(lines):
        if lines[i].startswith("--- "):
            old = lines[i][4:].split("\t")[0]
            new = lines[i + 1][4:].split("\t")[0]
            path = (new if old == "/dev/null" else old)[2:]
            i += 2
            continue
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", lines[i])
        if not m:
            i += 1
            continue
        old_start, old_n = int(m.group(1)), int(m.group(2) or 1)
        new_n = int(m.group(4) or 1)
        pre, n_old, n_new = [], 0, 0
        i += 1
        while i < len(lines) and (n_old < old_n or n_new < new_n):
            line = lines[i]
            if line.startswith("\\"):          # "\ No newline at end of file"
                i += 1
                continue
            tag, body = (line[:1] or " "), line[1:]
            assert tag in " +-", f"{path}: stray line in a hunk: {line!r}"
            if tag != "+":
                pre.append(body)
                n_old += 1
            if tag != "-":
                n_new += 1
            i += 1
        assert (n_old, n_new) == (old_n, new_n), f"{path} @@ -{old_start}: hunk line counts differ from its header"
        out.append((path, old_start, old_n, pre))
    return out


def _added_file(patch_text, path):
    """the text of a file the patch creates"""
    m = re.search(r"^\+\+\+ b/" + re.escape(path) + r"\n@@[^\n]*\n((?:\+[^\n]*\n)+)", patch_text, flags=re.M)
    assert m, f"{path} not created by the patch"
    return "".join(line[1:] + "\n" for line in m.group(1).splitlines())


def _header_decls():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(oem_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        p = params.strip()
        out[name] = 0 if p in ("", "void") else p.count(",") + 1
    return out, src


def test_patch_applies_to_the_reference_checkout():
    """Every hunk's pre-image (context and removed lines) is exactly what v0.10.3 holds at the hunk's stated lines, as
    recorded from a checkout by scripts/make_patch_fixture.py; the new file is new there."""
    ref = json.load(open(FIXTURE))
    hunks = patch_hunks(open(PATCH).read())
    created = [p for p, s, n, _ in hunks if (s, n) == (0, 0)]
    assert created == ref["created"]
    modified = [h for h in hunks if (h[1], h[2]) != (0, 0)]
    assert sorted({p for p, *_ in modified}) == sorted(ref["files"]), "the patch touches other files than recorded"
    recorded = {(p, h["old_start"], h["old_lines"]): h["sha256"] for p, f in ref["files"].items() for h in f["hunks"]}
    assert len(recorded) == len(modified), "the patch has other hunks than recorded: run scripts/make_patch_fixture.py"
    for path, start, n, pre in modified:
        key = (path, start, n)
        assert key in recorded, f"{path} @@ -{start},{n}: no recorded pre-image (run scripts/make_patch_fixture.py)"
        assert start + n - 1 <= ref["files"][path]["lines"], f"{path} @@ -{start},{n}: beyond the end of the file"
        assert lines_sha256(pre) == recorded[key], f"{path} @@ -{start},{n}: context differs from the reference"


def test_patch_is_a_diff_not_a_copy():
    """three lines of context around each call site; the only whole file is the new one"""
    text = open(PATCH).read()
    new_files = re.findall(r"^--- /dev/null\n\+\+\+ b/(\S+)", text, flags=re.M)
    assert new_files == ["src/em_gpu.rs"]
    context = [l for l in text.splitlines() if l.startswith(" ")]
    assert len(context) < 80, "context lines of the reference in the patch"


def test_extern_block_matches_the_header():
    rs = _added_file(open(PATCH).read(), "src/em_gpu.rs")
    decls, _ = _header_decls()
    block = re.search(r'unsafe extern "C" \{(.*?)\n\}', rs, flags=re.S).group(1)
    fns = re.findall(r"fn (oem_[a-z0-9_]+)\s*\((.*?)\)\s*(?:->\s*[^;]+)?;", block, flags=re.S)
    assert len(fns) >= 6
    for name, params in fns:
        assert name in decls, f"{name} is not declared by include/oarfish_em.h"
        n = len([p for p in params.split(",") if p.strip()])
        assert n == decls[name], f"{name}: {n} arguments in the Rust declaration, {decls[name]} in the header"


def test_repr_c_structs_match_the_header():
    rs = _added_file(open(PATCH).read(), "src/em_gpu.rs")
    _, hdr = _header_decls()

    def c_fields(struct):
        body = re.search(r"typedef struct\s*\{([^{}]*)\}\s*" + struct + r"\s*;", hdr, flags=re.S).group(1)
        return [re.sub(r"\[.*", "", f.strip().split()[-1]) for f in body.split(";") if f.strip()]

    def rs_fields(struct):
        body = re.search(r"pub struct " + struct + r"\s*\{(.*?)\n\}", rs, flags=re.S).group(1)
        return re.findall(r"pub ([a-z_0-9]+)\s*:", body)

    assert rs_fields("OemRunInfo") == c_fields("oem_run_info")
    assert rs_fields("OemStoreOpts") == c_fields("oem_store_opts")
    assert "oem_abi_version() } == %s" % re.search(r"#define OEM_ABI_VERSION (\d+)", open(HEADER).read()).group(1) in rs
