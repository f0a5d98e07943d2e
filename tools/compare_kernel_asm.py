#!/usr/bin/env python3
"""Compare two directories of device assembly files function by function.

    hipcc <FLAGS> -S --offload-device-only -o DIR/NAME.s SOURCE      (one file per unit and build, the same NAMEs in both)
    tools/compare_kernel_asm.py DIR_A DIR_B [--list]

A function is the text from its `_Z...:` label (announced by `.type NAME,@function`) to its `.Lfunc_endN:`; a kernel is a function that also has an
`.amdhsa_kernel` descriptor block, which is compared as well (registers, scratch, LDS). Local labels carry the index of
the function in its file (BB<n>_, JTI<n>_), which changes when a function before it comes or goes; they are compared
without it, and runs of white space as one blank. Per file: the functions of each side, those only one side has, and
those whose text or descriptor differs. Exit status 1 if a function both sides have differs. --list prints every kernel
name of side B per file."""
import os
import re
import sys

LABEL = re.compile(r'^(_Z\w+):')
END = re.compile(r'^\.Lfunc_end\d+:')
DESC = re.compile(r'^\s*\.amdhsa_kernel\s+(\S+)')
TYPE = re.compile(r'^\s*\.type\s+(\S+),@function')
INDEXED = re.compile(r'(BB|JTI)\d+_')


def norm(line):
    return re.sub(r'\s+', ' ', INDEXED.sub(r'\1_', line)).strip()


def parse(path):
    funcs, descs, name, desc, typed = {}, {}, None, None, set()
    for line in open(path, errors='replace'):
        if desc is not None:
            if line.strip() == '.end_amdhsa_kernel':
                desc = None
            else:
                descs[desc].append(norm(line))
            continue
        m = DESC.match(line)
        if m:
            desc = m.group(1)
            descs[desc] = []
            continue
        if name is None:
            m = TYPE.match(line)
            if m:
                typed.add(m.group(1))
            m = LABEL.match(line)
            if m and m.group(1) in typed:        # (a data symbol has a label too)
                name = m.group(1)
                funcs[name] = []
        elif END.match(line):
            name = None
        else:
            funcs[name].append(norm(line))
    return funcs, descs


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    if len(args) != 2:
        sys.exit(__doc__)
    listing = '--list' in sys.argv
    a_dir, b_dir = args
    names = sorted(set(f for f in os.listdir(a_dir) if f.endswith('.s')) | set(f for f in os.listdir(b_dir) if f.endswith('.s')))
    bad = 0
    for f in names:
        pa, pb = os.path.join(a_dir, f), os.path.join(b_dir, f)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f'{f}: only in {a_dir if os.path.exists(pa) else b_dir}')
            bad += 1
            continue
        (fa, da), (fb, db) = parse(pa), parse(pb)
        both = [k for k in fa if k in fb]
        text = [k for k in both if fa[k] != fb[k]]
        desc = [k for k in da if k in db and da[k] != db[k]]
        only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
        print(f'{f}: functions {len(fa)} / {len(fb)}, kernels {len(da)} / {len(db)}, lines of A {sum(1 for _ in open(pa))}, of B {sum(1 for _ in open(pb))}; '
              f'only in A {len(only_a)}, only in B {len(only_b)}, text differs {len(text)}, descriptor differs {len(desc)}')
        for k in only_a:
            print(f'  only in A: {k}')
        for k in only_b:
            print(f'  only in B: {k}')
        for k in text:
            print(f'  text differs: {k}')
        for k in desc:
            print(f'  descriptor differs: {k}')
        if listing:
            for k in sorted(db):
                print(f'  kernel: {k}')
        bad += len(text) + len(desc)
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
