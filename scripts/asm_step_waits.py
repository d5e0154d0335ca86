#!/usr/bin/env python3
"""Which waits on vector memory sit in the per-step loop of the team-recurrence kernels, and what do they wait for?

For every ``lstm_team_{fwd,bwd}_kernel`` of a gfx950 assembly listing the per-step loop is found from the control-flow
graph (the innermost natural loop around the step's LDS barrier, the ``s_barrier`` inside an ``ASMSTART`` region), and
every ``s_waitcnt vmcnt(N)`` inside it is printed with

* the vector-memory instructions that MAY be outstanding when it is reached: issued on some path since the last such
  wait, the way the compiler's wait-count insertion sees it (union over the predecessors, the loop's back edge and its
  entry included; ``vmcnt(N)`` keeps the youngest N of a straight line). ``pre:`` marks an instruction issued ahead of
  the step loop — a load left pending into the loop is what makes the compiler place a ``vmcnt(0)`` in every step;
* whether it sits in an ``ASMSTART`` region (written in the source) or was placed by the compiler;
* the instruction that follows it (the use the compiler protects).

A wait is classed by what was issued in its own straight line (its block, since the block's previous wait) or, inside
a loop nested in the step (a poll round, the t = 0 copy), anywhere in that loop: ``poll``
(a hand-off poll, ``buffer_load … sc1``), ``ctl`` (a control-block load or atomic: the abort flag, the team's
counters — the time-out and chain hand-shake paths), ``data`` (another load: the t = 0 path, a value loaded in the
step and used in it). A wait with no load in its straight line waits for something inherited from other paths:
``stale`` if an instruction from ahead of the step loop may be among it (a load left pending into the loop — the
defect), else ``merge``.

  hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S lstm_team_fwd.hip -o fwd.s
  python scripts/asm_step_waits.py fwd.s [bwd.s …] [--md] [--only SUBSTR]

``--md`` prints one table row per kernel (counts per class and the lines of the ``stale`` and store-draining waits)
instead of the full listing. It only reads listings; nothing is compiled or run.
"""
import re
import sys
from collections import Counter

PRODS = ('Bf16Mfma', 'SplitMfma', 'Valu4w', 'Valu8w')
NAME = re.compile(r'lstm_team_(fwd|bwd)_kernelILNS_4ProdE(\d)ELi(\d+)ELi(\d+)ELb([01])EE')
VMEM = re.compile(r'^(global_|buffer_|flat_|scratch_)(load|store|atomic)')
WAIT = re.compile(r'^s_waitcnt\b.*vmcnt\((\d+)\)')


def show(sym):
    m = NAME.search(sym)
    return '%s<%s, %s, %s, %s>' % (m.group(1), PRODS[int(m.group(2))], m.group(3), m.group(4),
                                   'true' if m.group(5) == '1' else 'false')


class Block:
    def __init__(self, label):
        self.label, self.ins, self.succ, self.pred = label, [], [], []   # ins: (line no, text, in asm region)


def blocks_of(lines, first):
    """Basic blocks of one kernel body with successor / predecessor edges (labels are the only branch targets)."""
    blocks = [Block('entry')]
    in_asm = False
    for no, ln in enumerate(lines, first):
        t = ln.strip()
        if t.startswith(';;#ASMSTART'):
            in_asm = True
        elif t.startswith(';;#ASMEND'):
            in_asm = False
        m = re.match(r'^(\.LBB\d+_\d+):', t)
        if m:
            blocks.append(Block(m.group(1)))
            continue
        t = t.split(';')[0].strip()
        if t and not t.startswith('.'):
            blocks[-1].ins.append((no, t, in_asm))
    by = {b.label: i for i, b in enumerate(blocks)}
    for i, b in enumerate(blocks):
        falls = True
        for _, t, _ in b.ins:
            op = t.split()[0]
            if op.startswith(('s_cbranch', 's_branch')):
                tgt = t.split()[-1]
                if tgt in by:
                    b.succ.append(by[tgt])
            if op in ('s_branch', 's_endpgm', 's_setpc_b64'):
                falls = False
        if falls and i + 1 < len(blocks):
            b.succ.append(i + 1)
        b.succ = list(dict.fromkeys(b.succ))
    for i, b in enumerate(blocks):
        for s in b.succ:
            blocks[s].pred.append(i)
    return blocks


def dominators(blocks):
    n = len(blocks)
    full = set(range(n))
    dom = [full.copy() for _ in range(n)]
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for i in range(1, n):
            ps = [dom[p] for p in blocks[i].pred]
            new = (set.intersection(*ps) if ps else set()) | {i}
            if new != dom[i]:
                dom[i], changed = new, True
    return dom


def step_loop(blocks):
    """Block indices of the innermost natural loop that holds the step's LDS barrier, its header, and the loops nested
    in it (the poll rounds, the t = 0 copy of h0); (None, None, []) if there is none."""
    dom = dominators(blocks)
    loops = {}
    for u, b in enumerate(blocks):
        for h in b.succ:
            if h in dom[u]:                               # back edge u → h
                body, work = {h, u}, [u]
                while work:
                    x = work.pop()
                    if x == h:
                        continue
                    for p in blocks[x].pred:
                        if p not in body:
                            body.add(p)
                            work.append(p)
                loops.setdefault(h, set()).update(body)
    bar = [i for i, b in enumerate(blocks) if any(t == 's_barrier' and a for _, t, a in b.ins)]
    best = None
    for h, body in loops.items():
        if any(x in body for x in bar) and (best is None or len(body) < len(loops[best])):
            best = h
    if best is None:
        return None, None, []
    inner = [body for h, body in loops.items() if h != best and body < loops[best]]
    return loops[best], best, inner


def outstanding(blocks):
    """Per block: the vector-memory instructions that may be outstanding on entry (a forward may-analysis)."""
    inn = [frozenset() for _ in blocks]
    out = [frozenset() for _ in blocks]

    def flow(i, s, seen=None):
        line = []                                         # issued in this block since its last vmcnt wait, in order
        keep = set(s)
        for no, t, _ in blocks[i].ins:
            w = WAIT.match(t)
            if w:
                if seen is not None:
                    seen[no] = (frozenset(keep) | frozenset(line), tuple(line))
                n = int(w.group(1))
                if len(line) >= n:                        # everything older than the youngest n has landed
                    keep, line = set(), line[len(line) - n:]
                # (fewer than n issued in this straight line: which of the inherited ones survive cannot be told)
            elif VMEM.match(t):
                line.append((no, t))
        return frozenset(keep) | frozenset(line)

    work = list(range(len(blocks)))
    while work:
        i = work.pop(0)
        s = frozenset().union(*[out[p] for p in blocks[i].pred]) if blocks[i].pred else frozenset()
        o = flow(i, s)
        inn[i] = s
        if o != out[i]:
            out[i] = o
            work.extend(x for x in blocks[i].succ if x not in work)
    seen = {}
    for i in range(len(blocks)):
        flow(i, inn[i], seen)
    return seen


def classify(pend, line, loop_lines, inner_ops):
    ops = [t for _, t in line] + inner_ops                # (inside a nested loop: what that loop issues)
    if any(t.startswith('buffer_load') and 'sc1' in t for t in ops):
        return 'poll'
    if any((t.startswith('global_load_dword ') and 'sc1' in t) or t.startswith('global_atomic') for t in ops):
        return 'ctl'
    if any('_load' in t for t in ops):
        return 'data'
    return 'stale' if any(no not in loop_lines for no, _ in pend) else 'merge'


def brief(pend, loop_lines):
    c = Counter(('' if no in loop_lines else 'pre:') + t.split()[0] + (' sc1' if 'sc1' in t else '') for no, t in pend)
    return ', '.join('%s%s' % (k, ' ×%d' % v if v > 1 else '') for k, v in sorted(c.items())) or '(nothing)'


def kernels(path):
    s = open(path).read().split('\n')
    i = 0
    while i < len(s):
        m = re.match(r'^(_Z\S+):', s[i])
        if m and NAME.search(m.group(1)) and not m.group(1).endswith('.kd'):
            j = i + 1
            while not s[j].startswith('.Lfunc_end'):
                j += 1
            yield m.group(1), s[i + 1:j], i + 2
            i = j
        i += 1


def main():
    args = sys.argv[1:]
    md = '--md' in args
    only = args[args.index('--only') + 1] if '--only' in args else None
    paths = [a for k, a in enumerate(args) if not a.startswith('--') and (k == 0 or args[k - 1] != '--only')]
    if md:
        print('| kernel | waits in the step loop | poll | ctl | data | merge | stale | stale or merge waits that may drain '
              'a store of the step: line (next instruction) |\n|---|---:|---:|---:|---:|---:|---:|---|')
    for path in paths:
        for sym, body, first in kernels(path):
            if only and only not in sym and only not in show(sym):
                continue
            blocks = blocks_of(body, first)
            loop, head, inner = step_loop(blocks)
            if loop is None:
                print(('| `%s` | no step loop found |' if md else '%s: no step loop found') % show(sym))
                continue
            seen = outstanding(blocks)
            loop_lines = {no for i in loop for no, _, _ in blocks[i].ins}
            rows = []
            for i in sorted(loop):
                ins = blocks[i].ins
                for k, (no, t, in_asm) in enumerate(ins):
                    if WAIT.match(t):
                        pend, line = sorted(seen[no][0]), seen[no][1]
                        nxt = ins[k + 1][1] if k + 1 < len(ins) else '(block end)'
                        inner_ops = [x for body in inner if i in body for j in body for _, x, _ in blocks[j].ins
                                     if VMEM.match(x)]
                        rows.append((no, t, in_asm, blocks[i].label, classify(pend, line, loop_lines, inner_ops),
                                     pend, nxt))
            cls = Counter(r[4] for r in rows)
            if md:
                drains = [r for r in rows if not r[2] and r[4] in ('stale', 'merge') and
                          any('store' in t and no in loop_lines for no, t in r[5])]
                print('| `%s` | %d | %d | %d | %d | %d | %d | %s |' % (
                    show(sym), len(rows), cls['poll'], cls['ctl'], cls['data'], cls['merge'], cls['stale'],
                    ', '.join('%d (`%s`)' % (r[0], r[6].split()[0]) for r in drains) or 'none'))
                continue
            print('%s  (%s)\n  step loop: header %s, %d blocks; %d vmcnt waits: %s' % (
                show(sym), path, blocks[head].label, len(loop), len(rows), dict(cls)))
            for no, t, in_asm, label, c, pend, nxt in rows:
                print('  %6d %-10s %-22s %-5s %-8s next: %s\n           may be outstanding: %s' % (
                    no, label, t, c, 'ASM' if in_asm else 'compiler', nxt, brief(pend, loop_lines)))
            print()


if __name__ == '__main__':
    main()
