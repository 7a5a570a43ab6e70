"""Instruction counts of every closest-hit walk in a trace kernel's ISA (`make asm` output), by loop
level: the traversal step (the blocks at the depth of the loop that reads the node record), the
leaf site one level down, the triangle loop below that.  A kernel with one walk per query kind
 lists one row set per walk, in code order.
Usage: python tools/walk_isa.py gpu-ray-tracer_amd/build/rt_kernels.s [kernel-substring]"""
import collections
import re
import sys

src = open(sys.argv[1]).read().split('\n')
pat = sys.argv[2] if len(sys.argv) > 2 else 'trace_kernelILi0ELb1ELi180E'
st = [i for i, l in enumerate(src) if re.match(r'^_Z\S*' + pat + r'\S*:', l)][0]
en = [i for i in range(st, len(src)) if src[i].startswith('.Lfunc_end')][0]
body = src[st:en]


def kind(op):
    if op.startswith('v_mov'): return 'v_mov'
    if op.startswith(('v_readlane', 'v_writelane')): return 'lane'
    if op.startswith('v_'): return 'valu'
    if op.startswith(('s_cbranch', 's_branch')): return 'branch'
    if op.startswith(('s_waitcnt', 's_nop')): return 'wait'
    if op.startswith(('s_load', 's_buffer')): return 'smem'
    if op.startswith('s_'): return 'salu'
    if op.startswith('ds_'): return 'lds'
    return 'vmem'


# blocks: (first line, innermost loop's header); loops: header -> parent loop's header
blocks, parent = [], {}
for i, l in enumerate(body):
    if not re.match(r'^(\.LBB\d+_\d+:|; %bb\.\d+:)', l):
        continue
    m = re.search(r'in Loop: Header=(BB\d+_\d+)', l)
    if m:
        blocks.append((i, m.group(1)))
        continue
    lab = re.match(r'^\.L(BB\d+_\d+):', l)
    own, up = None, None
    for j in range(i, min(i + 16, len(body))):               # a loop header: its parents, then its own line
        c = body[j]
        if j > i and not c.lstrip().startswith(';'): break
        q = re.search(r'Parent Loop (BB\d+_\d+)', c)
        if q: up = q.group(1)
        if re.search(r'This (Inner )?Loop Header', c): own = lab.group(1) if lab else None; break
    if own: parent[own] = up
    blocks.append((i, own))
bounds = [b[0] for b in blocks] + [len(body)]


def level(h, top):
    """0 for loop `top`, 1 for its child loops, ...; None outside it"""
    n = 0
    while h is not None:
        if h == top: return n
        h = parent.get(h); n += 1
    return None


# the walks: loop headers whose own block reads a node record's child pair
walks = [h for k, (i, h) in enumerate(blocks) if h and body[i].startswith('.L' + h + ':') and h in parent and
         any('ds_read_b64' in x and 'offset:48' in x for x in body[i:bounds[k + 1]])]
print('kernel', pat, 'walks', len(walks))
for w, top in enumerate(walks):
    per = collections.defaultdict(collections.Counter)
    for k, (i, h) in enumerate(blocks):
        lvl = level(h, top)
        if lvl is None: continue
        for l in body[i + 1:bounds[k + 1]]:
            s = l.strip()
            if l.startswith('\t') and s and not s.startswith(('.', ';')):
                per[min(lvl, 3)][kind(s.split()[0])] += 1
    for lvl, name in enumerate(('traversal step', 'leaf site', 'triangle loop', 'deeper')):
        c = per.get(lvl)
        if c:
            print('walk %d  %-15s %5d  %s' % (w, name, sum(c.values()), dict(sorted(c.items()))))
