#!/usr/bin/env python3
"""Compare two device assembly files of one source, kernel by kernel:  tools/dev_kernel_diff.py OLD.s NEW.s

Per kernel symbol: "identical" when the instruction streams agree after dropping comments and directives and numbering the labels in order of
appearance; otherwise the resource metadata of both sides and the opcodes whose counts differ (OLD -> NEW).  Exit status 1 if any kernel differs
or exists on one side only.  The .s files come from the Makefile's HIPFLAGS plus `--cuda-device-only -S` (README, tool index).  CPU only."""
import collections
import re
import sys

META = ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')


def parse(path):
    """{kernel symbol: (instruction lines with labels renumbered, {metadata key: value})}"""
    lines = open(path).read().split('\n')
    names = [m.group(1) for m in (re.match(r'\s*\.amdhsa_kernel\s+(\S+)', x) for x in lines) if m]
    body, cur = {}, None
    for x in lines:
        x = x.split(';')[0].rstrip()
        m = re.match(r'(\S+):$', x)
        if m and m.group(1) in names:
            cur = body.setdefault(m.group(1), [])
        elif re.match(r'\.Lfunc_end\d+:$', x):
            cur = None
        elif cur is not None and x.strip() and (not x.strip().startswith('.') or x.strip().endswith(':')):
            cur.append(x.strip())
    meta, entry = {}, {}
    for x in lines[lines.index('amdhsa.kernels:') + 1 if 'amdhsa.kernels:' in lines else len(lines):]:
        if x.startswith('  - ') or not x.startswith(' '):
            if '.name' in entry:
                meta[entry['.name']] = entry
            entry = {}
            if not x.startswith(' '):
                break
        m = re.match(r'(?:    |  - )(\.\w+):\s*(\S+)$', x)
        if m:
            entry[m.group(1)] = m.group(2)
    out = {}
    for name, ins in body.items():
        labels = {}
        for x in ins:
            for lab in re.findall(r'\.L\w+', x):
                labels.setdefault(lab, f'.L{len(labels)}')
        out[name] = ([re.sub(r'\.L\w+', lambda m: labels[m.group(0)], x) for x in ins], {k: meta.get(name, {}).get(k, '?') for k in META})
    return out


def main(old_path, new_path):
    old, new = parse(old_path), parse(new_path)
    differ = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f'{name}: only in {"NEW" if name in new else "OLD"}'); differ += 1
            continue
        (oi, om), (ni, nm) = old[name], new[name]
        if oi == ni and om == nm:
            print(f'{name}: identical ({len(oi)} lines)')
            continue
        differ += 1
        print(f'{name}: DIFFERS ({len(oi)} -> {len(ni)} lines)')
        print('    ' + ', '.join(f'{k} {om[k]} -> {nm[k]}' for k in META))
        oc, nc = (collections.Counter(x.split()[0] for x in ins if not x.endswith(':')) for ins in (oi, ni))
        delta = [f'{op} {oc[op]} -> {nc[op]}' for op in sorted(set(oc) | set(nc)) if oc[op] != nc[op]]
        print('    opcode counts: ' + ('; '.join(delta) if delta else 'the same (order or registers differ)'))
    print(f'{len(set(old) | set(new)) - differ} of {len(set(old) | set(new))} kernels identical')
    return 1 if differ else 0


if __name__ == '__main__':
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
