"""Compares two builds' gfx950 assembly (the `.s` that `hipcc -save-temps` keeps) kernel by kernel.

    python tools/dev/isa_diff.py OLD.s NEW.s

Every kernel of OLD is matched with the kernel of the same demangled name in NEW (or the one that gained a trailing
`false` template argument: the per-agent flag at its default; or the box / constraint form of step_kernel or prox_kernel
that was a kernel of a name of its own, in either direction) and their instruction streams are compared with labels
and symbol names masked.  Prints the kernels that differ and the counts.  No GPU needed.
"""
import re,subprocess,sys
def funcs(path):
    out={}; cur=None; buf=[]
    for ln in open(path):
        m=re.match(r"^(_Z\w+):\s*(;.*)?$",ln)
        if m and cur is None:
            cur=m.group(1); buf=[]; continue
        if cur is not None:
            if ln.startswith(".Lfunc_end"):
                out[cur]=buf; cur=None; continue
            s=ln.split(";")[0].strip()
            if not s or s.startswith("."): continue
            buf.append(s)
    return out
old=funcs(sys.argv[1]); new=funcs(sys.argv[2])
names=list(old)+list(new)
dem=dict(zip(names,subprocess.check_output(["c++filt"]+names,text=True).split("\n")))
base=lambda n: dem[n].split("(")[0].replace("void ","")
newby={}
for n in new:
    b=base(n); newby[b]=n
for n in new:   # the per-agent flag at its default, stripped -- only where that name is not taken
    b=base(n); s=re.sub(r"<false>$","",re.sub(r", false>$",">",b))
    if s!=b and (b.endswith("false>")): newby.setdefault("STRIP:"+s,n)
def old_name(b):   # a box or constraint form that had a kernel name of its own: step_kernel<1, 0, true, BoxTab, ConTab> was
    m=re.fullmatch(r"(.*::)?(step|prox)_kernel<(.*?)(?:, )?(mpc::BoxTab)?(?:, )?(mpc::ConTab)?>",b)   # step_kernel_box_con<1, 0>
    if not m: return b
    ns,k,args,box,con=m.groups(); sfx="_box"*bool(box)+"_con"*bool(con)
    if con: args=args[:-len(", true")]
    return (ns or "")+(k+"_kernel"+sfx if k=="step" else k+sfx+"_kernel")+("<%s>"%args if args else "")
for n in new: newby.setdefault("STRIP:"+old_name(base(n)),n)
mask=lambda x: re.sub(r"\.L\w+","LBL",re.sub(r"_Z\w+","SYM",x))
same=diff=0
for n in old:
    if "kernel" not in dem[n]: continue
    k=newby.get("STRIP:"+old_name(base(n))) or newby.get(base(n))
    if k is None: print("missing",dem[n][:80]); continue
    ma=[mask(x) for x in old[n]]; mb=[mask(x) for x in new[k]]
    if ma==mb: same+=1
    else: diff+=1; print("DIFF",base(n),"->",base(k),len(ma),len(mb))
print(same,"kernels with identical instruction streams,",diff,"differ")
