import re,sys
# usage: isa_diff.py [--rename REGEX=REPL] [--hidden-args OLD=NEW] <name> ...
#   compares /tmp/isa/base/<name>.s with /tmp/isa/new/<name>.s (hipcc --offload-device-only -S of the parent's and of this tree's source)
#   --rename REGEX=REPL    applied to the NEW side's text: a template that gained a defaulted parameter mangles every instantiation anew
#                          (e.g. '(xcorr_fused_n4096_foldILb.ELb.ELb.ELb.E)Lb0E(EEv)=\1\2')
#   --hidden-args OLD=NEW  FusedParams grew at its END by NEW - OLD bytes: the offset of the implicit arguments behind it (OLD in the
#                          parent, NEW here, e.g. 0x1e0=0x1f0) is the one literal that moves
# Basic-block labels carry the function's number in the file (.LBB<function>_<block>): compared without it.
rename=None; hidden=None; names=[]
args=sys.argv[1:]
while args:
    a=args.pop(0)
    if a=='--rename': rename=args.pop(0).split('=',1)
    elif a=='--hidden-args': hidden=args.pop(0).split('=',1)
    else: names.append(a)
def funcs(path,new):
    out={}; cur=None
    for line in open(path):
        if new and rename: line=re.sub(rename[0],rename[1],line)
        l=line.split(';')[0].rstrip()
        s=l.strip()
        if not s or s.startswith('.file') or s.startswith('.loc'): continue
        m=re.match(r'^(_Z\w+):',l)
        if m:
            cur=m.group(1); out[cur]=[]; continue
        if s.startswith('.end_amdhsa_kernel') or l.startswith('.Lfunc_end') or s.startswith('.section'):
            cur=None
        if cur:
            if re.match(r's_load_dword\w* .*0x1[89a-f][0-9a-f]$',s) or re.match(r's_load_dword\w* .*0x2[0-9a-f][0-9a-f]$',s): s='HIDDEN_ARG_LOAD'
            if s.startswith('.amdhsa_kernarg_size'): continue
            if new and hidden and s.endswith(', '+hidden[1]): s=s[:-len(hidden[1])]+hidden[0]
            s=re.sub(r'\.LBB\d+_','.LBB_',s)
            out[cur].append(re.sub(r'__hip_cuid_\w+','CUID',s))
    return out
for f in names:
    a=funcs('/tmp/isa/base/%s.s'%f,False); b=funcs('/tmp/isa/new/%s.s'%f,True)
    nd=0
    for k in a:
        if a[k]!=b.get(k):
            nd+=1
            d=sum(1 for x,y in zip(a[k],b.get(k,[])) if x!=y)
            print('  DIFF',f,k[:90],len(a[k]),len(b.get(k,[])),'lines differing',d)
    print(f,'kernels',len(a),'different',nd, 'missing/new', set(a)^set(b))
