"""SGPR spill census of a trace kernel (`make asm` output): ISA metadata (SGPR / VGPR spills,
scratch) and the v_readlane / v_writelane spill restores and saves by loop, so that the cost of
the spills is placed: per group (the persistent group loop), per state-machine iteration (one
per wave query), or per traversal step.  The traversal stack's own lane moves (M0 / SGPR-indexed)
are left out.  Usage: python tools/spill_census.py gpu-ray-tracer_amd/build/rt_kernels.s [kernel-substring]"""
import collections
import re
import sys

src = open(sys.argv[1]).read()
pat = sys.argv[2] if len(sys.argv) > 2 else 'trace_kernelILi0ELb1ELi180E'
for b in src.split('  - .agpr_count'):
    n = re.search(r'\.name:\s+(\S+)', b)
    if n and pat in n.group(1):
        print(n.group(1))
        for k in ('sgpr_count', 'sgpr_spill_count', 'vgpr_count', 'vgpr_spill_count', 'private_segment_fixed_size'):
            print('  %-28s %s' % (k, re.search(r'\.%s:\s+(\d+)' % k, b).group(1)))
lines = src.split('\n')
st = [i for i, l in enumerate(lines) if re.match(r'^_Z\S*' + pat + r'\S*:', l)][0]
en = [i for i in range(st, len(lines)) if lines[i].startswith('.Lfunc_end')][0]
depth, per = 0, collections.Counter()
n_inst = 0
for i in range(st, en):
    l = lines[i]
    m = re.match(r'^(?:\.LBB\d+_\d+:|; %bb\.\d+:)(.*)', l)
    if m:
        d = re.search(r'in Loop: Header=\S+ Depth=(\d+)', m.group(1))
        depth = int(d.group(1)) if d else 0
        if not d:                                              # a loop header: its parents' lines, then its own depth
            for j in range(i, min(i + 16, en)):
                if j > i and not lines[j].lstrip().startswith(';'):
                    break
                h = re.search(r'This (?:Inner )?Loop Header: Depth=(\d+)', lines[j])
                if h:
                    depth = int(h.group(1))
                    break
        continue
    s = l.strip()
    if not s or s.startswith(('.', ';')):
        continue
    n_inst += 1
    op = s.split()[0]
    if op == 'v_readlane_b32' and not re.search(r', s\d+$', s):          # not an SGPR-indexed (stack) read
        per[(depth, 'restore')] += 1
    if op == 'v_writelane_b32' and 'm0' not in s:
        per[(depth, 'save')] += 1
print('instructions', n_inst)
# Loop names by depth relative to the traversal step, whose depth is read from the listing (the loop
# whose header block reads a node record's child pair): the kernels differ in how many loops enclose
# it (the hot kernel has a loop over sample rounds between the group loop and the state machine).
step = None
for i in range(st, en):
    if 'ds_read_b64' in lines[i] and 'offset:48' in lines[i]:
        for j in range(i, max(st, i - 40), -1):
            m = re.search(r'This (?:Inner )?Loop Header: Depth=(\d+)', lines[j])
            if m:
                step = int(m.group(1))
                break
        if step is not None:
            break
rel = {-3: 'group loop', -2: 'sample rounds', -1: 'state machine (per wave query)', 0: 'traversal step',
       1: 'leaf site', 2: 'triangle loop'}


def name(d):
    if d == 0:
        return 'kernel prologue/epilogue'
    if step is None:
        return 'loop'
    if d == 1 and step >= 3:
        return 'group loop'
    return rel.get(d - step, 'outer loop' if d < step else 'deeper loops')


for (d, k), v in sorted(per.items()):
    print('  depth %d %-32s %-8s %d (static)' % (d, name(d), k, v))
