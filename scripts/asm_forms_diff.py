#!/usr/bin/env python3
"""Are the team-recurrence kernels of two builds the same machine code?

Compares every ``lstm_team_{fwd,bwd}_kernel`` instantiation of an OLD gfx950 assembly listing (one translation unit,
kernels named by the former ``<MT, KS, F32, VAR>`` parameters) with the NEW listings (kernels named by their form,
``<Prod, rows, KS, libm>``): the text between a kernel's label and its ``.Lfunc_end``, without comments, with mangled
symbol names numbered by first appearance and the function index taken out of the ``.LBB<n>_`` labels, is hashed
and compared, and so are the four resource figures of the kernel's metadata record. It only hashes and compares.

  hipcc <the build's flags> --cuda-device-only -S old/lstm_team.hip -o old.s      (likewise fwd.s, bwd.s)
  python scripts/asm_forms_diff.py old.s fwd.s bwd.s [--md]

Prints one row per old kernel (old name, new name, identical, vgpr / agpr / LDS bytes / scratch bytes) and exits 1 if
a kernel that has a new counterpart differs from it, or if a new kernel has no old counterpart.
"""
import hashlib
import re
import sys

PRODS = ('Bf16Mfma', 'SplitMfma', 'Valu4w', 'Valu8w')
FIGS = ('.vgpr_count', '.agpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size')
OLD = re.compile(r'lstm_team_(fwd|bwd)_kernelILi(\d+)ELi(\d+)ELb([01])ELi(\d+)EE')
NEW = re.compile(r'lstm_team_(fwd|bwd)_kernelILNS_4ProdE(\d)ELi(\d+)ELi(\d+)ELb([01])EE')


def form_key(sym):
    """(direction, prod, rows, H, libm) of a kernel symbol of either naming, or None."""
    m = NEW.search(sym)
    if m:
        return m.group(1), PRODS[int(m.group(2))], int(m.group(3)), 128 * int(m.group(4)), m.group(5) == '1'
    m = OLD.search(sym)
    if not m:
        return None
    mt, ks, f32, var = int(m.group(2)), int(m.group(3)), m.group(4) == '1', int(m.group(5))
    lg_rows, rest = divmod(var, 32)         # the former packing: waves + 4·libm + 32·log2(rows)
    libm, waves = divmod(rest, 4)
    if waves == 0:
        return m.group(1), PRODS[1 if f32 else 0], 16 * mt, 128 * ks, False
    return m.group(1), PRODS[1 + waves], 1 << lg_rows, 128 * ks, libm == 1


def kernels(path):
    """{form key: (symbol, body hash, resource figures)} of a listing."""
    s = open(path).read()
    figs = {}
    meta = s[s.index('.amdgpu_metadata'):]
    for rec in meta.split('\n  - ')[1:]:
        name = re.search(r'^\s*\.name:\s+(\S+)', rec, re.M)
        if name:
            figs[name.group(1)] = tuple(int(re.search(r'^\s*\%s:\s+(\d+)' % f, rec, re.M).group(1)) for f in FIGS)
    out = {}
    for m in re.finditer(r'^(_Z\S+):[ \t]*(;.*)?$', s, re.M):
        key = None if m.group(1).endswith('.kd') else form_key(m.group(1))
        if key is None:
            continue
        body = s[m.end():s.index('.Lfunc_end', m.end())]
        body = re.sub(r';.*', '', body)
        body = re.sub(r'\.LBB\d+_', '.LBB_', body)
        names = {}
        body = re.sub(r'_Z\w+', lambda x: names.setdefault(x.group(0), 'SYM%d' % len(names)), body)
        body = '\n'.join(ln.rstrip() for ln in body.split('\n') if ln.strip())
        out[key] = (m.group(1), hashlib.sha256(body.encode()).hexdigest(), figs[m.group(1)])
    return out


def show(key):
    d, prod, rows, h, libm = key
    return f'{d} <{prod}, {rows}, {h // 128}, {str(libm).lower()}>'


def main():
    args = [a for a in sys.argv[1:] if a != '--md']
    md = '--md' in sys.argv
    old = kernels(args[0])
    new = {}
    for p in args[1:]:
        new.update(kernels(p))
    bad = 0
    if md:
        print('| old | new | identical | vgpr | agpr | LDS bytes | scratch bytes |\n|---|---|---|---|---|---|---|')
    for key in sorted(old):
        sym, h, figs = old[key]
        oldname = '%s <%s>' % (key[0], ', '.join(OLD.search(sym).groups()[1:]))
        if key in new:
            same = new[key][1] == h and new[key][2] == figs
            bad += not same
            row = (oldname, show(key), 'yes' if same else 'NO', *figs) if same else \
                  (oldname, show(key), 'NO', *('%d → %d' % (a, b) for a, b in zip(figs, new[key][2])))
        else:
            row = (oldname, 'dropped', '-', *figs)
        print(('| ' + ' | '.join(map(str, row)) + ' |') if md else '  '.join(f'{str(c):<30}' if i < 2 else f'{str(c):>9}'
                                                                            for i, c in enumerate(row)))
    extra = sorted(set(new) - set(old))
    for key in extra:
        print('no old counterpart:', show(key))
    kept = len(set(new) & set(old))
    print(f'\n{len(old)} old kernels, {len(new)} new, {kept} in both, {kept - bad} identical, '
          f'{len(old) - kept} dropped, {len(extra)} without an old counterpart')
    sys.exit(1 if bad or extra else 0)


if __name__ == '__main__':
    main()
