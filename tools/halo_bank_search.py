import numpy as np, itertools, collections
GROUPS=[[0,1,2,3,12,13,14,15,20,21,22,23,24,25,26,27],[4,5,6,7,8,9,10,11,16,17,18,19,28,29,30,31]]
GROUPS+= [[l+32 for l in g] for g in GROUPS]
def evalf(KS,CINB,MF,f,pitch_pad,TD=4,TH=8,TW=8):
    NVV=CINB//16
    HH,HW=TH+KS-1,TW+KS-1
    PW=((HW+pitch_pad-1)//pitch_pad)*pitch_pad
    G=max(1,NVV//2 if MF==32 else NVV//4)
    tot=0;n=0;worst=0
    for kd,kh,kw in itertools.product(range(KS),repeat=3):
        for i in range(64//MF):
            for g in range(G):
                for grp in GROUPS:
                    slots=collections.Counter()
                    for lane in grp:
                        lvb=(lane>>5) if MF==32 else (lane>>4)
                        lv=lvb+(2*g if MF==32 else 4*g)
                        r=i*MF+(lane&(MF-1)); tw=r%TW; th=(r//TW)%TH; td=r//(TW*TH)
                        hd,hh,hw=td+kd,th+kh,tw+kw
                        hv=(hd*HH+hh)*PW+hw
                        pv=lv^(f(hd,hh,hw,hv)%NVV)
                        slots[((hv*CINB+pv*16)//16)%16]+=1
                    c=max(slots.values()); tot+=c;n+=1;worst=max(worst,c)
    return tot/n,worst,PW
def worst_way(addr_of):
    """worst number of distinct 16-byte addresses on one 16-byte bank slot (256-byte row) over the four lane groups of a ds_read_b128; addr_of(n, q) for lane 16 q + n"""
    w=0
    for grp in GROUPS:
        slots=collections.defaultdict(set)
        for lane in grp:
            a=addr_of(lane&15,lane>>4); slots[(a//16)%16].add(a)
        w=max(w,max(len(v) for v in slots.values()))
    return w
def check_mf16():
    """the v_mfma_f32_16x16x32_bf16 fragment reads (lane = 16 q + n reads k-vector q of voxel / pixel / weight row n): worst conflict over every tap, 1 = conflict-free"""
    # conv2d_halo_kernel: 512-byte pixels, pitch 26, 2 x 8 pixel fragments; slot ^ swizzle(row, column); candidates: the 32x32x16 swizzle, the one in use
    for name,swz,pix in (("(c&7)|(r&1)<<3, lane n -> (n>>3, n&7)",lambda r,c:(c&7)|((r&1)<<3),lambda n:(n>>3,n&7)),
                         ("(r&1)|(c&7)<<1, lane n -> (n&1, n>>1)",lambda r,c:(r&1)|((c&7)<<1),lambda n:(n&1,n>>1))):
        w=max(worst_way(lambda n,q:((2*i+pix(n)[0]+kh)*26+8*j+pix(n)[1]+kw)*512+(((4*m+q)^swz(2*i+pix(n)[0]+kh,8*j+pix(n)[1]+kw))<<4))
              for kh in range(3) for kw in range(3) for i in range(4) for j in range(3) for m in range(8))
        print("conv2d_halo 16x16x32, swizzle %s: worst %d-way"%(name,w))
    # conv3d_halo_col_kernel: 64-byte voxels, pitch 10, swizzle (hw>>1)&3 as stored by the loaders; fragment = two rows of eight voxels, the column order is searched
    for perm in itertools.permutations(range(3)):
        col=lambda n,perm=perm:sum(((n>>perm[b])&1)<<b for b in range(3))
        w=max(worst_way(lambda n,q:((2*f+(n>>3)+kh)*10+col(n)+kw)*64+((q^(((col(n)+kw)>>1)&3))<<4)) for kh in range(3) for kw in range(3) for f in range(4))
        print("conv3d_halo_col 16x16x32, column bits (b0,b1,b2) = lane bits %s: worst %d-way"%(perm,w))
    chan=lambda n,s:16*(n>>3)+8*((n>>2)&1)+4*s+(n&3)
    w=max(worst_way(lambda n,q:chan(n,s)*64+((q^((-(chan(n,s)//4))&3))<<4)) for s in range(2))
    print("conv3d_halo_col 16x16x32, weight rows 16(n>>3)+8(n>>2&1)+4s+(n&3): worst %d-way"%w)
import sys
if "--mf16" in sys.argv:
    check_mf16(); sys.exit(0)
for (KS,CINB,MF) in [(3,64,32),(7,64,16),(3,128,32),(3,32,32),(3,64,32)]:
    best=[]
    for pad in (1,2,4):
        for a,b,c,sh in itertools.product(range(4),range(4),range(4),(0,1,2,3)):
            f=lambda hd,hh,hw,hv,a=a,b=b,c=c,sh=sh: a*hh+b*hd+((hw+c*hh)>>sh)
            avg,w,PW=evalf(KS,CINB,MF,f,pad)
            best.append((avg,w,pad,PW,a,b,c,sh))
        for sh in (0,1,2,3,4):
            f=lambda hd,hh,hw,hv,sh=sh: hv>>sh
            avg,w,PW=evalf(KS,CINB,MF,f,pad); best.append((avg,w,pad,PW,'hv>>',sh,0,0))
    best.sort(key=lambda t:(t[0],t[3]))
    print((KS,CINB,MF),best[:4])
