#!/usr/bin/env python3
"""Instruction mix per basic block of one kernel of an assembly listing: the blocks that hold matrix or exp instructions.

    hipcc <the Makefile's flags> --cuda-device-only -S csrc/fa_mfma16_kernel.hip -o k.s
    python tools/isa_hot_tile.py k.s <mangled kernel name>

Prints, per basic block (labelled, or a fall-through block `%bb.N`), the MFMA, v_exp and v_cvt_pk counts and the other VALU by opcode: the hot tile of the 16x16x32 forward is the
block with 32 v_exp (DESIGN 6.3d, row "hot tile")."""
import re,sys
def blocks(path,name):
    t=open(path).read()
    st=t.index(name+':'); en=t.index('.Lfunc_end',st)
    out=[]; cur=['entry',[]]
    for l in t[st:en].splitlines()[1:]:
        c=l.split(';')[0].strip()
        if l.startswith('.LBB') or l.startswith('; %bb.'):  # (a fall-through block has no label of its own, only the comment)
            out.append(cur); cur=[l.split(':')[0].lstrip('; '),[]]
        elif c and not c.startswith('.') : cur[1].append(c)
    out.append(cur); return out
def summarize(path,name):
    for lab,ins in blocks(path,name):
        mf=sum(i.startswith('v_mfma') for i in ins); ex=sum(i.startswith('v_exp') for i in ins)
        if mf==0 and ex==0: continue
        cv=sum(i.startswith('v_cvt_pk') for i in ins)
        valu=[i for i in ins if i.startswith('v_') and not i.startswith('v_mfma')]
        other=[i.split()[0] for i in valu if not i.startswith('v_exp') and not i.startswith('v_cvt_pk')]
        from collections import Counter
        print(f"{lab:12s} mfma {mf:3d} v_exp {ex:3d} cvt_pk {cv:3d} other VALU {len(other):3d} {dict(Counter(other))}  ds {sum(i.startswith('ds_') for i in ins)} salu {sum(i.startswith('s_') for i in ins)}")
if __name__=='__main__':
    summarize(sys.argv[1],sys.argv[2])
