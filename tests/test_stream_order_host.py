"""The stream-order contract without a GPU: every stream-taking prototype of include/gmr_amd.h has a case in
tests/test_gpu_stream_order.py, and in gmr_amd/csrc/api.hip -- the only place kernels are launched from -- every launch, every
asynchronous copy / memset and every stream-ordered allocation reachable from those entries names the call's own stream, and none
of those functions calls a blocking or default-stream runtime function.  What the header says about synchronising entries is
what the code does and what profiles/stream_order.json recorded on the GPU."""
import ast
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gmr_amd.h")
API_HIP = os.path.join(ROOT, "gmr_amd", "csrc", "api.hip")
CASE_FILE = os.path.join(ROOT, "tests", "test_gpu_stream_order.py")
PROFILE = os.path.join(ROOT, "profiles", "stream_order.json")

HEADER_STAGED_UP_TO_KIB = 512   # the largest pageable table the header says is staged without waiting (the sweep's last such size)
STREAM_EXPRS = {"st", "static_cast<hipStream_t>(stream)", "s->st"}   # the three styles the call sites use
FORBIDDEN = ("hipMemcpy", "hipMemset", "hipDeviceSynchronize", "hipMalloc", "hipFree")
# Preprocessor blocks left out of the check, with the reason.
ALLOWED_BLOCKS = {
    "GMR_IK_STAMPS": "diagnostic builds only (per-phase cycle stamps): allocates and clears its counters once, never in the shipped library",
}
# (unit, call) pairs whose stream argument is not one of STREAM_EXPRS, with the reason; checked separately below.
ALLOWED_CALLS = {
    ("CallScratch", "hipFreeAsync"): "the destructor frees on CallScratch::st, which both allocation sites set to the call's stream (checked: every `.st =` assigns `st`)",
}


# ------------------------------------------------------------------ the case table and the header, read as text
def _module_literal(path, name):
    """Keys of the dict / elements of the set assigned to ``name`` at the top level of a Python file (no import: the file needs torch)."""
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            v = node.value
            elems = v.keys if isinstance(v, ast.Dict) else v.elts
            return {ast.literal_eval(e) for e in elems}
    raise AssertionError(f"{name} not found in {path}")


def strip_c(text):
    """C / C++ text with comments and string / character literals blanked (same length, newlines kept)."""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            j = text.find("\n", i)
            j = n if j < 0 else j
            out.append(" " * (j - i)); i = j
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append("".join(ch if ch == "\n" else " " for ch in text[i:j])); i = j
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(c + " " * (j - i - 1) + c); i = j + 1
        else:
            out.append(c); i += 1
    return "".join(out)


def stream_prototypes(header_path=HEADER):
    text = strip_c(open(header_path).read())
    protos = re.findall(r"\b(gmr_\w+)\s*\(([^;{}()]*)\)\s*;", text)
    return {name for name, args in protos if re.search(r"void\s*\*\s*stream\b", args)}


def header_synchronising_entries(header_path=HEADER):
    """The entries the header's stream-order paragraph names as synchronising the stream before they return."""
    text = " ".join(re.sub(r"^\s*\*", " ", ln) for ln in open(header_path).read().split("\n"))
    m = re.search(r"entries that synchronise\s+`stream`\s+before they return[^:]*:\s*([^.]*)\.", text)
    assert m, "the header's stream-order paragraph does not list the synchronising entries"
    return set(re.findall(r"gmr_\w+", m.group(1)))


# ------------------------------------------------------------------ api.hip as units (functions and structs) with their bodies
def _preprocess(text):
    """Comment-free text in which preprocessor directives are blanked: whole directives outside function bodies, the directive's
    `#define NAME(args)` head inside them (the body of an in-function #define is code that runs: the launch macros).  Blocks
    guarded by a macro of ALLOWED_BLOCKS are blanked altogether."""
    lines = strip_c(text).split("\n")
    out, depth, skip, i = [], 0, [], 0
    while i < len(lines):
        ln = lines[i]
        if re.match(r"\s*#", ln):
            grp = [ln]
            while grp[-1].rstrip().endswith("\\") and i + 1 < len(lines):
                i += 1
                grp.append(lines[i])
            m = re.match(r"\s*#\s*(ifdef|ifndef|if|endif)\b\s*(\w*)", ln)
            if m and m.group(1) != "endif":
                skip.append(m.group(1) == "ifdef" and m.group(2) in ALLOWED_BLOCKS)
            inside = any(skip)
            if m and m.group(1) == "endif" and skip:
                skip.pop()
            keep_tail = depth > 1 and not inside   # (depth 1 = the namespace / extern "C" block)
            body = re.sub(r"^\s*#\s*define\s+\w+(\([^)]*\))?", "", ln) if re.match(r"\s*#\s*define\b", ln) else ""
            grp[0] = body
            out.extend((g.rstrip().rstrip("\\") if keep_tail else "") for g in grp)
        else:
            if any(skip):
                out.append("")
            else:
                out.append(ln)
                depth += ln.count("{") - ln.count("}")
        i += 1
    return "\n".join(out)


def units(path=API_HIP):
    """name -> text (header and body) of every function and struct defined directly inside the namespace / extern "C" blocks."""
    text = _preprocess(open(path).read())
    res, kinds, stmt, start = {}, [], 0, None   # kinds: 'c' container, 'u' unit, 'b' block inside a unit
    for i, ch in enumerate(text):
        if ch == "{":
            if all(k == "c" for k in kinds):
                head = text[stmt:i].strip()
                if re.match(r"(namespace\b|extern\b)", head):
                    kinds.append("c"); stmt = i + 1
                else:
                    kinds.append("u"); start = stmt
            else:
                kinds.append("b")
        elif ch == "}":
            k = kinds.pop()
            if k == "u":
                head = text[start:text.index("{", start)].strip()
                m = re.match(r"(?:struct|class|union|enum)\s+(\w+)", head) or re.search(r"([A-Za-z_]\w*)\s*\(", head)
                if m:   # (overloads share a name: their texts are checked as one unit)
                    res[m.group(1)] = res.get(m.group(1), "") + text[start:i + 1] + "\n"
            if all(k == "c" for k in kinds):
                stmt = i + 1
        elif ch == ";" and all(k == "c" for k in kinds):
            stmt = i + 1
    assert not kinds, "unbalanced braces"
    return res


def reachable(us, entry):
    seen, todo = set(), [entry]
    while todo:
        u = todo.pop()
        if u in seen:
            continue
        seen.add(u)
        body = us[u]
        todo.extend(v for v in us if v not in seen and re.search(r"\b" + re.escape(v) + r"\b", body))
    return seen


def call_args(text, at):
    """The top-level arguments of the call whose '(' is at text[at]."""
    depth, args, cur = 0, [], []
    for ch in text[at:]:
        if ch in "([{":
            depth += 1
            if depth == 1:
                continue
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                args.append("".join(cur))
                return [re.sub(r"\s+", "", a) if "(" not in a else re.sub(r"\s+", " ", a).strip().replace("> (", ">(") for a in args]
        if ch == "," and depth == 1:
            args.append("".join(cur)); cur = []
        else:
            cur.append(ch)
    raise AssertionError("unterminated call")


def check_api(path=API_HIP, entries=None):
    """Problems found in the functions reachable from the stream-taking entries (an empty list: none), and per entry whether it
    reaches a stream synchronisation."""
    us = units(path)
    entries = sorted(stream_prototypes() if entries is None else entries)
    problems, syncs = [], {}
    reach = {e: reachable(us, e) for e in entries if e in us}
    problems += [f"{e}: not defined in api.hip" for e in entries if e not in us]
    for name in sorted(set().union(*reach.values())):
        body = us[name]
        for m in re.finditer(r"\b(hipLaunchKernelGGL|hip\w+Async)\s*\(", body):
            fn = m.group(1)
            args = call_args(body, m.end() - 1)
            stream = args[4] if fn == "hipLaunchKernelGGL" else args[-1]
            if (name, fn) in ALLOWED_CALLS:
                continue
            if stream not in STREAM_EXPRS:
                problems.append(f"{name}: {fn} on `{stream}`, not on the call's stream")
            elif stream == "s->st" and not name.startswith("gmr_session"):
                problems.append(f"{name}: {fn} on a session's stream outside session code")
            elif stream == "st" and not re.search(r"hipStream_t\s+st\s*(=\s*static_cast<hipStream_t>\(stream\)\s*)?[;,)]", body):
                problems.append(f"{name}: {fn} on `st`, which is not the call's stream here (no `hipStream_t st` parameter or cast of `stream`)")
        for m in re.finditer(r"(\.|->)st\s*=\s*([^;]*);", body):
            if m.group(2).strip() != "st":
                problems.append(f"{name}: a scratch block's stream is set to `{m.group(2).strip()}`")
        for f in FORBIDDEN:
            if re.search(r"\b" + f + r"\s*\(", body):
                problems.append(f"{name}: calls {f}(), which blocks or works on the default stream")
    for e, r in reach.items():
        syncs[e] = any(re.search(r"\bhipStreamSynchronize\s*\(", us[u]) for u in r)
    return problems, syncs


# ------------------------------------------------------------------ the tests
def test_every_stream_taking_entry_has_a_case():
    protos = stream_prototypes()
    assert len(protos) == 27 and "gmr_motion_sample" in protos and "gmr_session_step" not in protos
    assert protos == _module_literal(CASE_FILE, "CASES")


def test_api_launches_copies_and_allocations_name_the_calls_stream():
    problems, _ = check_api()
    assert not problems, "\n".join(problems)


def test_the_checker_sees_what_it_should():
    """The parser finds the units and call sites it is meant to check (a parser that found nothing would pass everything)."""
    us = units()
    for name in ("prepare_ik_launch", "ik_run", "launch_ik", "launch_ik_group", "motion_run", "track_run", "report_run", "fk_launch", "bvh_fk_launch",
                 "scratch_alloc", "CallScratch", "gmr_motion_sample", "gmr_bvh_parse_motion_device"):
        assert name in us, name
    r = reachable(us, "gmr_ik_solve")
    assert {"ik_run", "prepare_ik_launch", "launch_ik_variant", "launch_ik", "scratch_alloc", "CallScratch"} <= r and "gmr_session_step" not in r
    assert "gmr_fk_shape" in reachable(us, "gmr_fk") and "fk_launch" in reachable(us, "gmr_fk")
    n_launch = sum(len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us[u])) for u in set().union(*(reachable(us, e) for e in stream_prototypes())))
    assert n_launch >= 30, n_launch   # 40 sites today, the launch macros' bodies included
    assert len(re.findall(r"\bhipLaunchKernelGGL\s*\(", us["launch_ik"])) == 6 and "hipMalloc" not in us["prepare_ik_launch"]
    body = "f(a, (gmr::k<A, B>), dim3(n), dim3(64), lds, static_cast<hipStream_t> (stream), x, y)"
    assert call_args(body, 1)[4] == "lds" and call_args(body, 1)[5] == "static_cast<hipStream_t>(stream)"


def test_synchronising_entries_are_the_ones_the_header_names():
    named = header_synchronising_entries()
    assert named == _module_literal(CASE_FILE, "SYNCHRONISES")
    _, syncs = check_api()
    assert {e for e, s in syncs.items() if s} == named


def test_profile_agrees_with_the_header():
    """profiles/stream_order.json (written on an MI355X by tests/test_gpu_stream_order.py): every entry, and for each what the
    header promises -- the call returned while its producer was still running unless it is one of the synchronising entries."""
    prof = json.load(open(PROFILE))
    assert prof["spin_calibration"]["ms_per_cycle"] > 0
    ent = prof["entries"]
    assert set(ent) == stream_prototypes()
    named = header_synchronising_entries()
    for e, rec in ent.items():
        assert rec["deterministic"] and rec["decoys_differ"] and not rec["vacuous"] and rec["equals_serial"], e
        assert rec["control_sees_decoy"] and rec["two_streams_equal_serial"], e
        assert rec["returned_before_producer"] == (e not in named), e
        assert 5.0 <= rec["spin_ms"] <= 250.0 and rec["spin_ms"] >= min(250.0, 10.0 * rec["serial_ms"]) - 0.01, e
    for e, rec in prof["large_host_tables"].items():   # a 1 MiB pageable table: as correct, but the call waited for the stream
        assert e.split("/")[0] in ent and rec["deterministic"] and rec["decoys_differ"] and not rec["vacuous"] and rec["equals_serial"], e
        assert not rec["returned_before_producer"], e
    sweep = prof["pageable_copy_sweep_gmr_fk_min_height"]
    assert all(r["equals_serial"] and not r["vacuous"] for r in sweep)
    limit = HEADER_STAGED_UP_TO_KIB * 1024 + 8   # (a table of n clips holds n + 1 offsets)
    assert max(r["table_bytes"] for r in sweep) == limit and all(r["returned_before_producer"] for r in sweep if r["table_bytes"] <= limit)
    assert f"up to {HEADER_STAGED_UP_TO_KIB} KiB" in " ".join(open(HEADER).read().split())
