#!/usr/bin/env python3
"""Per-block instruction mix of the hot region (reachable between HOT markers) of one kernel: hot_loop_mix.py <file.s> <kernel> [--classes]

--classes: the instructions that are neither arithmetic nor a memory access -- 32-bit vector ALU, s_nop, s_waitcnt -- by cause, per
block (a block belongs to one wavefront role's path or to both; the mix line above it tells which):
  addr      v_add_u32 / v_lshl* / v_mad_u32 / v_and / v_bfe / v_sub: address or index arithmetic (on loop-invariant per-lane values in
            the element phases: the access is `base + constant`, or `base + 8 * (a field of the lane's packed constants)`)
  select    v_cndmask_b32 and the v_cmp_*_u32 / v_xor that feed it: a select on a lane or role predicate
  copy      v_mov_b32 / v_mov_b64 / v_accvgpr: a constant placed in a register, or a copy at a control-flow join
  nop-mfma  s_nop directly behind a v_mfma (its result is the next instruction's DPP, LDS-store or VALU source)
  nop-other any other s_nop (behind a DPP move, a write of exec / vcc, a lane read)
  wait-bar  s_waitcnt directly in front of s_barrier (the phase's stores drain)
  wait-all  s_waitcnt lgkmcnt(0) elsewhere (everything issued so far has to arrive: first use of the last load, or earlier than needed)
  wait-cnt  a counted s_waitcnt (independent loads stay in flight)"""
import os, re, sys
from collections import Counter
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asm_mix import classify
path, name = sys.argv[1], sys.argv[2]
CLASSES = "--classes" in sys.argv[3:]
body, on = [], False
for ln in open(path):
    m = re.match(r"^(_Z\w+):", ln)
    if m:
        on = name in m.group(1); body = [] if on else body
        continue
    if on:
        body.append(ln)
        if ln.startswith(".Lfunc_end"): break
labels = {}
for i, b in enumerate(body):
    m = re.match(r"^(\.LBB\d+_\d+):", b)
    if m: labels[m.group(1)] = i
starts = [i + 1 for i, b in enumerate(body) if "LPVMPC_HOT_BEGIN" in b]
seen = set(); work = list(starts)
while work:
    i = work.pop()
    while i < len(body) and i not in seen:
        seen.add(i); b = body[i]
        if "LPVMPC_HOT_END" in b or "LPVMPC_HOT_BEGIN" in b: break
        if b.startswith("\t") and not b.strip().startswith((".", ";")):
            op = b.split()[0]
            if op == "s_endpgm": break
            m = re.search(r"(\.LBB\d+_\d+)", b) if op.startswith(("s_cbranch", "s_branch")) else None
            if m and m.group(1) in labels: work.append(labels[m.group(1)])
            if op == "s_branch": break
        i += 1
# group by basic block in text order
def cause(op, text, prev_op, next_op):
    if op == "s_nop": return "nop-mfma" if prev_op.startswith("v_mfma") else "nop-other"
    if op == "s_waitcnt":
        if next_op == "s_barrier": return "wait-bar"
        return "wait-all" if re.search(r"lgkmcnt\(0\)", text) and "vmcnt" not in text else ("wait-all" if re.search(r"lgkmcnt\(0\)", text) else "wait-cnt")
    if classify(op) != "valu32": return None
    if op.startswith(("v_cndmask", "v_cmp", "v_xor")): return "select"
    if op.startswith(("v_mov", "v_accvgpr", "v_bfrev")): return "copy"
    if op.startswith(("v_add_u32", "v_add_co", "v_lshl", "v_lshr", "v_ashr", "v_mad_u32", "v_mad_i32", "v_mul_i32", "v_mul_u32", "v_mul_lo", "v_and", "v_or", "v_bfe", "v_sub", "v_bfi")): return "addr"
    return "other"
cur, blocks, causes = "start", {}, {}
order = []
ins = [(i, body[i].split()[0], body[i]) for i in sorted(seen) if body[i].startswith("\t") and not body[i].strip().startswith((".", ";"))]
around = {i: (ins[n - 1][1] if n else "", ins[n + 1][1] if n + 1 < len(ins) else "") for n, (i, _, _) in enumerate(ins)}
for i in sorted(seen):
    b = body[i]
    m = re.match(r"^(\.LBB\d+_\d+):", b)
    if m: cur = m.group(1)
    if b.startswith("\t") and not b.strip().startswith((".", ";")):
        if cur not in blocks: blocks[cur] = Counter(); causes[cur] = Counter(); order.append(cur)
        blocks[cur][classify(b.split()[0])] += 1
        c = cause(b.split()[0], b, *around[i])
        if c: causes[cur][c] += 1
        if b.split()[0].startswith('ds_'):
            blocks[cur]['lds_' + ('rd' if 'read' in b.split()[0] else 'wr')] += 1
tot = Counter()
for k in order:
    c = blocks[k]; tot += c
    print("%-12s %4d  %s" % (k, sum(v for kk, v in c.items() if not kk.startswith('lds_')), " ".join("%s %d" % kv for kv in sorted(c.items()))))
    if CLASSES and causes[k]: print("%-12s       causes: %s" % ("", " ".join("%s %d" % kv for kv in sorted(causes[k].items()))))
print("total", sum(v for kk, v in tot.items() if not kk.startswith('lds_')), dict(tot))
if CLASSES:
    ct = Counter()
    for k in order: ct += causes[k]
    print("causes", sum(ct.values()), dict(sorted(ct.items())))
