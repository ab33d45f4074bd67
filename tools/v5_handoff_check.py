#!/usr/bin/env python3
"""Lint of the comb walker's hand-off from the ISA (dev tool + CPU test, no GPU needed): what stage 2 of k_v5_walk relies on
when it hands a strip's record to its right-hand neighbour, and what no GPU test can see (the window is a few hundred cycles).

The record leaves with one 16-byte sc1 store in the slot's head.  In an interior slot it is then waited for with
`s_waitcnt vmcnt(KEEP)`, KEEP a hand count of the vector-memory operations the source issues behind that store (vmcnt counts
loads, stores and atomics of a wave together, in issue order; flat_* excepted).  A wrong count passes every test: the record is
simply no longer waited for.  The scan reads the assembly of the build with region marks (tools/v5_asm.sh, -DSMX_V5_MARK) as
functions, basic blocks and a control-flow graph (labels, s_branch, s_cbranch_*, fall-through), and holds, per k_v5_walk:

  R1  every hand-written `s_waitcnt vmcnt(N)`, N > 0, is reached from exactly one `s2rows begin` mark, on every graph path from
      that mark at least N vector-memory instructions lie in front of it, the `s2head` region in front of the mark holds exactly
      one 16-byte sc1 buffer store, and no further such store lies between `s2head end` and the wait
  R2  there is such a wait, and the N of a function are {S2_KEEP} (QP = 0) or {S2_KEEP - BH/2} (QP = 1) of the source
  R3  no flat_* and no scratch_* instruction (they would break the issue-order premise of vmcnt)
  R4  each `s2head` region has one ds_add_u32 (tile 2 is released to stage 1), a `s_waitcnt lgkmcnt(0)` lies behind the last
      ds_read* on every path to it, and no ds_read* lies between it and `s2head end`
  R5  every buffer instruction on the descriptor (SGPR quad) of a record store carries sc1, and there is a 16-byte sc1 load
  R6  the build without marks (the product's code) has, per function, the same vector-memory opcodes, ds_add_u32, s_barrier
      and hand-written counted waits; R3 and R5 hold there too; the flags of v5_asm.sh are CXXFLAGS of csrc/Makefile
  R7  the KEEP site is the only inline-assembly vmcnt( with a count other than a literal 0 under csrc/

It proves a count on the marked build and equal histograms on the product build, not the product's ISA path by path; the
record-0 store of the stage-1 role, the flag publish behind the barrier and the ring walker (vmcnt(0) drains: R7 only) are
outside it.

  python tools/v5_handoff_check.py [extra -D flags ...]      exit status 1 + a list of findings (function, line, rule)
"""
import collections, glob, os, re, shlex, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_matching_cuda_amd", "csrc")
WALKER = re.compile(r"k_v5_walkILi(\d+)ELi(\d+)EE")
Finding = collections.namedtuple("Finding", "func line rule msg")
Ins = collections.namedtuple("Ins", "line op text hand")      # op "MARK": a region mark, text its name; hand: inside inline assembly


class Func:
    def __init__(self, name):
        self.name, self.ins, self.labels, self.broken = name, [], {}, []

    def link(self):
        """successors and predecessors of every instruction; a branch the graph cannot follow lands in self.broken"""
        n = len(self.ins)
        self.succ = [[] for _ in range(n)]
        for i, x in enumerate(self.ins):
            nxt = [i + 1] if i + 1 < n else []
            if x.op == "s_branch" or x.op.startswith("s_cbranch_"):
                tgt = self.labels.get(x.text.split()[1])
                if tgt is None or tgt >= n:
                    self.broken.append(x)
                    tgt = None
                self.succ[i] = ([] if tgt is None else [tgt]) + (nxt if x.op != "s_branch" else [])
            elif x.op in ("s_endpgm", "s_setpc_b64", "s_swappc_b64"):
                if x.op != "s_endpgm":
                    self.broken.append(x)
            else:
                self.succ[i] = nxt
        self.pred = [[] for _ in range(n)]
        for i, ss in enumerate(self.succ):
            for s in ss:
                self.pred[s].append(i)
        return self

    def marks(self, name):
        return [i for i, x in enumerate(self.ins) if x.op == "MARK" and x.text == name]

    def reach(self, start, stops=(), back=False):
        """the instructions on a path from `start` (or to it, back=True); a path ends at a stop, which is part of the set"""
        edges, seen, todo = (self.pred if back else self.succ), {start}, [start]
        while todo:
            for j in edges[todo.pop()]:
                if j not in seen:
                    seen.add(j)
                    if j not in stops:
                        todo.append(j)
        return seen

    def between(self, a, b, stops=()):
        """the instructions on a path from a to b that passes no stop"""
        stops = set(stops)
        return self.reach(a, stops | {b}) & self.reach(b, stops | {a}, back=True)


def parse(asm_lines, fragment=None):
    """the functions of an assembly text; fragment=name: the text is the body of one function without its header"""
    funcs, cur, hand = [], (Func(fragment) if fragment else None), False
    for no, raw in enumerate(asm_lines, 1):
        s = raw.strip()
        if s.startswith(";;#ASMSTART"):
            hand = True
        elif s.startswith(";;#ASMEND"):
            hand = False
        m = re.match(r";\s*MARK\s+(.*\S)", s)
        if m and cur is not None:
            cur.ins.append(Ins(no, "MARK", m.group(1), True))
            continue
        s = s.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"([A-Za-z_.$][\w.$]*):", s)
        if m:
            if m.group(1).startswith(".Lfunc_end"):
                if cur is not None and not fragment:
                    funcs.append(cur.link())
                    cur = None
            elif m.group(1).startswith(".L"):
                if cur is not None:
                    cur.labels[m.group(1)] = len(cur.ins)
            elif not fragment and re.search(r";\s*@" + re.escape(m.group(1)), raw):
                cur = Func(m.group(1))
            continue
        if s.startswith(".") or cur is None:
            continue
        cur.ins.append(Ins(no, s.split()[0], s, hand))
    if fragment:
        funcs.append(cur.link())
    return funcs


def waits(x):
    """the counters an s_waitcnt sets, by name"""
    if x.op != "s_waitcnt":
        return {}
    w = {k: int(v, 0) for k, v in re.findall(r"(vmcnt|lgkmcnt|expcnt)\((\w+)\)", x.text)}
    m = re.match(r"s_waitcnt\s+(0x[0-9a-fA-F]+|\d+)\s*$", x.text)
    if m:                                                      # the gfx9 immediate: vmcnt [3:0] + [15:14], expcnt [6:4], lgkmcnt [11:8]
        v = int(m.group(1), 0)
        w = {"vmcnt": (v & 15) | ((v >> 14) & 3) << 4, "expcnt": (v >> 4) & 7, "lgkmcnt": (v >> 8) & 15}
    return w


def is_vmem(x):
    return x.op.startswith(("buffer_", "global_"))


def counts_in_vmcnt(x):
    # the cache maintenance operations are left out of the count: fewer counted can only turn a pass into an alarm
    return is_vmem(x) and not x.op.startswith(("buffer_wbl2", "buffer_inv", "buffer_gl"))


def is_rec_store(x):
    return x.op == "buffer_store_dwordx4" and " sc1" in x.text


def descriptor(x):
    m = re.search(r"s\[(\d+):(\d+)\]", x.text) if x.op.startswith("buffer_") else None
    return (int(m.group(1)), int(m.group(2))) if m and int(m.group(2)) - int(m.group(1)) == 3 else None


def counted_waits(f):
    return [i for i, x in enumerate(f.ins) if x.hand and waits(x).get("vmcnt", 0) > 0]


def min_vmem(f, a, b):
    """the least number of vector-memory instructions on a graph path from a to b (both excluded); None: no path"""
    dist, todo = {a: 0}, collections.deque([a])               # 0-1 breadth-first search
    while todo:
        i = todo.popleft()
        if i == b:
            continue
        for j in f.succ[i]:
            c = dist[i] + (1 if counts_in_vmcnt(f.ins[j]) and j != b else 0)
            if c < dist.get(j, 1 << 30):
                dist[j] = c
                (todo.append if c > dist[i] else todo.appendleft)(j)
    return dist.get(b)


def r1(f):
    out, notes = [], []
    for x in f.broken:
        out.append(Finding(f.name, x.line, "R1", f"`{x.text}` leaves the function's graph: the paths cannot be walked"))
    heads, rows, ends = f.marks("s2head begin"), f.marks("s2rows begin"), f.marks("s2head end")
    for w in counted_waits(f):
        W, n = f.ins[w], waits(f.ins[w])["vmcnt"]
        site = f"vmcnt({n}) at line {W.line}"
        bs = sorted(f.reach(w, set(heads) | set(rows), back=True) & set(rows))
        if len(bs) != 1:
            out.append(Finding(f.name, W.line, "R1", f"{site}: reached from {len(bs)} `s2rows begin` marks "
                               f"(lines {[f.ins[b].line for b in bs]}), not from exactly one"))
            continue
        b = bs[0]
        k = min_vmem(f, b, w)
        if k < n:
            out.append(Finding(f.name, W.line, "R1", f"{site}: a path from `s2rows begin` (line {f.ins[b].line}) issues only {k} "
                               f"vector-memory instructions: the wait no longer covers the record store"))
        else:
            notes.append(f"{f.name}: {site}: N = {n}, counted minimum {k} from `s2rows begin` at line {f.ins[b].line}"
                         + (" (waits for more than the record)" if k > n else ""))
        es = sorted(f.reach(b, set(ends) | set(rows) - {b}, back=True) & set(ends))
        hs = sorted(f.reach(es[0], set(heads) | set(ends) - {es[0]}, back=True) & set(heads)) if len(es) == 1 else []
        if len(es) != 1 or len(hs) != 1:
            out.append(Finding(f.name, f.ins[b].line, "R1", f"{site}: `s2rows begin` is not led to by exactly one `s2head` region"))
            continue
        e, h = es[0], hs[0]
        st = sorted(i for i in f.between(h, e, heads) if is_rec_store(f.ins[i]))
        if len(st) != 1:
            out.append(Finding(f.name, f.ins[h].line, "R1", f"{site}: the `s2head` region at line {f.ins[h].line} holds {len(st)} "
                               f"16-byte sc1 buffer stores, not exactly one record store"))
        for i in sorted(f.between(e, w, heads)):
            if is_rec_store(f.ins[i]):
                out.append(Finding(f.name, f.ins[i].line, "R1", f"{site}: a 16-byte sc1 store lies between `s2head end` "
                                   f"(line {f.ins[e].line}) and the wait: the count is not anchored behind it"))
    return out, notes


def expected_keep(qp, csrc=CSRC):
    src = open(os.path.join(csrc, "smx_agg_v5.hip")).read() + open(os.path.join(csrc, "smx_agg_v5.h")).read()
    keep = int(re.search(r"constexpr\s+int\s+S2_KEEP\s*=\s*(\d+)\s*;", src).group(1))
    bh = int(re.search(r"constexpr\s+int\s+BH\s*=\s*(\d+)\s*;", src).group(1))
    return keep - bh // 2 if qp else keep


def r2(f, expect=None):
    out = []
    ns = sorted({waits(f.ins[w])["vmcnt"] for w in counted_waits(f)})
    line = f.ins[0].line if f.ins else 0
    if not ns:
        out.append(Finding(f.name, line, "R2", "no hand-written counted wait: nothing was checked"))
    elif expect is not None and ns != [expect]:
        out.append(Finding(f.name, f.ins[counted_waits(f)[0]].line, "R2", f"the counted waits have N = {ns}, the source's constants give {expect}"))
    for what, n in (("`s2rows begin` mark", len(f.marks("s2rows begin"))), ("`s2head begin` mark", len(f.marks("s2head begin"))),
                    ("vector-memory instruction", sum(map(is_vmem, f.ins))), ("ds_* instruction", sum(x.op.startswith("ds_") for x in f.ins))):
        if n == 0:
            out.append(Finding(f.name, line, "R2", f"no {what}: nothing was checked"))
    return out


def r3(f):
    return [Finding(f.name, x.line, "R3", f"`{x.text}`: {x.op.split('_')[0]}_* instructions do not keep vmcnt's issue order")
            for x in f.ins if x.op.startswith(("flat_", "scratch_"))]


def r4(f):
    out = []
    heads, ends = f.marks("s2head begin"), f.marks("s2head end")
    for h in heads:
        es = sorted(f.reach(h, set(heads) - {h} | set(ends)) & set(ends))
        if len(es) != 1:
            out.append(Finding(f.name, f.ins[h].line, "R4", f"`s2head begin` reaches {len(es)} `s2head end` marks, not exactly one"))
            continue
        e = es[0]
        region = f.between(h, e, heads)
        adds = sorted(i for i in region if f.ins[i].op == "ds_add_u32")
        if len(adds) != 1:
            out.append(Finding(f.name, f.ins[h].line, "R4", f"the `s2head` region holds {len(adds)} ds_add_u32, not exactly one"))
            continue
        a = adds[0]
        # (instruction, an LDS read is outstanding) over the paths from the mark to the add
        seen, todo = {(h, False)}, [(h, False)]
        while todo:
            i, dirty = todo.pop()
            if i == a:
                continue
            for j in f.succ[i]:
                if j not in region:
                    continue
                x = f.ins[j]
                d = True if x.op.startswith("ds_read") else False if waits(x).get("lgkmcnt") == 0 else dirty
                if (j, d) not in seen:
                    seen.add((j, d))
                    todo.append((j, d))
        if (a, True) in seen:
            out.append(Finding(f.name, f.ins[a].line, "R4", "ds_add_u32 releases tile 2 on a path on which no `s_waitcnt lgkmcnt(0)` "
                               "lies behind the last ds_read*"))
        for i in sorted(f.between(a, e, heads)):
            if f.ins[i].op.startswith("ds_read"):
                out.append(Finding(f.name, f.ins[i].line, "R4", f"`{f.ins[i].text}` reads LDS behind the ds_add_u32 of line {f.ins[a].line} "
                                   "that released tile 2"))
    return out


def r5(f):
    out = []
    quads = {descriptor(x) for x in f.ins if is_rec_store(x)} - {None}
    line = f.ins[0].line if f.ins else 0
    if not quads:
        out.append(Finding(f.name, line, "R5", "no 16-byte sc1 buffer store: the record stores have lost their sc1 bit"))
    for x in f.ins:
        if x.op.startswith("buffer_") and descriptor(x) in quads and " sc1" not in x.text:
            out.append(Finding(f.name, x.line, "R5", f"`{x.text}` uses the descriptor s[{descriptor(x)[0]}:{descriptor(x)[1]}] of a record "
                               "store without sc1 (a hand-off access without the bit, or the compiler has reused the SGPR quad for "
                               "another descriptor: then this rule needs a better notion of the hand-off descriptor)"))
    if not any(x.op == "buffer_load_dwordx4" and " sc1" in x.text for x in f.ins):
        out.append(Finding(f.name, line, "R5", "no `buffer_load_dwordx4 ... sc1`: the hand-in load has lost its sc1 bit"))
    return out


def histogram(f):
    h = collections.Counter(x.op for x in f.ins if is_vmem(x) or x.op in ("ds_add_u32", "s_barrier"))
    h.update(f"hand-written s_waitcnt vmcnt({waits(f.ins[w])['vmcnt']})" for w in counted_waits(f))
    return h


def r6_functions(marked, product):
    """R6 on the walker functions of the two builds (lists of Func)"""
    out = []
    pm = {f.name: f for f in product}
    for f in marked:
        p = pm.pop(f.name, None)
        if p is None:
            out.append(Finding(f.name, 0, "R6", "the product build has no such function"))
            continue
        a, b = histogram(f), histogram(p)
        for k in sorted(set(a) | set(b)):
            if a[k] != b[k]:
                out.append(Finding(f.name, 0, "R6", f"{k}: {a[k]} in the marked build, {b[k]} in the product build"))
    for p in pm.values():
        out.append(Finding(p.name, 0, "R6", "the marked build has no such function"))
    for p in product:
        out += [x._replace(rule="R6/" + x.rule) for x in r3(p) + r5(p)]
    return out


def flags_of_script(text):
    """the compile flags of the hipcc line of v5_asm.sh (continuation lines joined), without what names files"""
    m = re.search(r"^\S*hipcc\s+((?:.*\\\n)*.*)$", text.replace("\r", ""), re.M)
    toks = shlex.split(m.group(1).replace("\\\n", " "), posix=True) if m else []
    toks = toks[:toks.index(">/dev/null")] if ">/dev/null" in toks else toks
    out, skip = [], False
    for i, t in enumerate(toks):
        if skip:
            skip = False
        elif t == "-o":
            skip = True
        elif t in ("-c", "--save-temps", "$@") or t.endswith(".hip"):
            pass
        else:
            out.append(t)
    return out


def flags_of_makefile(text):
    m = re.search(r"^CXXFLAGS\s*[:+?]?=\s*((?:.*\\\n)*.*)$", text, re.M)
    return m.group(1).replace("\\\n", " ").split() if m else []


def r6_flags(script_text, makefile_text):
    norm = lambda t: t.replace("$(ARCH)", "gfx950").replace("$(ROOT)", "$ROOT")
    mk = [norm(t) for t in flags_of_makefile(makefile_text) if t not in ("-Wall", "-Wno-unused-function", "$(EXTRA)")]
    sh = [norm(t) for t in flags_of_script(script_text) if t not in ("-DSMX_V5_MARK", "$MARK")]
    if not mk or not sh:
        return [Finding("tools/v5_asm.sh", 0, "R6", "the compile flags could not be read from the script or the Makefile")]
    if mk != sh:
        return [Finding("tools/v5_asm.sh", 0, "R6", f"flags differ from CXXFLAGS of csrc/Makefile: only in the script "
                        f"{[t for t in sh if t not in mk]}, only in the Makefile {[t for t in mk if t not in sh]}"
                        + ("" if sorted(mk) != sorted(sh) else " (order)"))]
    return []


def r7(sources):
    """sources: {file name: text}; an inline-assembly string with vmcnt( and a count other than a literal 0"""
    out, sites = [], []
    for name, text in sorted(sources.items()):
        for m in re.finditer(r"(?:\basm\b|__asm__|__asm\b)[^;]*?\"[^\"]*vmcnt\(([^)]*)\)", text):
            if m.group(1).strip() != "0":
                no = text.count("\n", 0, m.start()) + 1
                stmt = text[m.start():text.find(";", m.start())]
                sites.append((name, no, m.group(1), stmt))
    for name, no, cnt, stmt in sites:
        if not (os.path.basename(name) == "smx_agg_v5.hip" and cnt == "%0" and re.search(r'"n"\s*\(\s*KEEP\s*\)', stmt)):
            out.append(Finding(name, no, "R7", f"a counted wait vmcnt({cnt}) in inline assembly that the lint does not know"))
    if not any(os.path.basename(n) == "smx_agg_v5.hip" and c == "%0" for n, _, c, _ in sites):
        out.append(Finding("smx_agg_v5.hip", 0, "R7", "the KEEP site was not found"))
    return out


def walkers(funcs):
    return [f for f in funcs if WALKER.search(f.name)]


def check_marked(funcs, csrc=CSRC):
    """R1 - R5 on the functions of the marked build -> (findings, notes)"""
    out, notes = [], []
    ws = walkers(funcs)
    if not ws:
        out.append(Finding("-", 0, "R2", "no k_v5_walk function in the assembly: nothing was checked"))
    for f in ws:
        a, b = r1(f)
        out += a + r2(f, expected_keep(int(WALKER.search(f.name).group(2)), csrc)) + r3(f) + r4(f) + r5(f)
        notes += b
    return out, notes


def assembly(extra, mark):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "v5.s")
        subprocess.check_call([os.path.join(ROOT, "tools", "v5_asm.sh"), out, *extra], env=dict(os.environ, V5_ASM_MARK="1" if mark else "0"))
        return open(out).read().split("\n")


def main(extra):
    marked, product = parse(assembly(extra, True)), parse(assembly(extra, False))
    out, notes = check_marked(marked)
    out += r6_functions(walkers(marked), walkers(product))
    out += r6_flags(open(os.path.join(ROOT, "tools", "v5_asm.sh")).read(), open(os.path.join(CSRC, "Makefile")).read())
    out += r7({os.path.relpath(p, ROOT): open(p).read() for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p)})
    for n in notes:
        print(n)
    for x in out:
        print(f"FINDING {x.rule} {x.func} line {x.line}: {x.msg}")
    print(f"{len(walkers(marked))} walker functions, {len(notes)} counted waits covered, {len(out)} findings")
    return 1 if out else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
