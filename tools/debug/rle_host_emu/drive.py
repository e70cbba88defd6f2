"""Driver of emu.cpp (see its header): enc / dec / tile compare the emulated kernels with tests/dicom_rle_model.py."""
import sys, struct, subprocess, os
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "..", "..", "tests")]
import numpy as np
import dicom_rle_model as m
import tempfile
EMU = os.path.join(HERE, "emu")
D = tempfile.mkdtemp() + os.sep
def enc(imgs):
    n,rows,cols=imgs.shape; planes=imgs.dtype.itemsize
    imgs.tofile(D+"in.bin")
    subprocess.run([EMU,"e",str(planes),str(rows),str(cols),str(n),D+"in.bin",D+"out.bin"],check=True)
    b=open(D+"out.bin","rb").read(); out=[]; p=0
    for i in range(n):
        s=struct.unpack("<I",b[p:p+4])[0]; out.append(b[p+4:p+4+s]); p+=4+s
    return out
def dec(frames, rows, cols, bits):
    N=rows*cols; step=bits//8; nsegf=step
    blob=b"".join(frames); segs=b""; off=0; t0=0; nseg=0
    for i,f in enumerate(frames):
        head=struct.unpack("<16I",f[:64]); offs=list(head[1:1+nsegf])+[len(f)]
        for k in range(nsegf):
            ln=offs[k+1]-offs[k]
            segs+=struct.pack("<QQII", off+offs[k], i*N*step+(nsegf-1-k), ln, t0); t0+=(ln+2047)//2048; nseg+=1
        off+=len(f)
    open(D+"segs.bin","wb").write(segs); open(D+"frames.bin","wb").write(blob)
    subprocess.run([EMU,"d",str(N),str(step),str(nseg),D+"segs.bin",D+"frames.bin",D+"img.bin",str(len(frames))],check=True)
    b=open(D+"img.bin","rb").read()
    ss=np.frombuffer(b[:nseg*4],np.uint32)
    img=np.frombuffer(b[nseg*4:],np.uint8 if bits==8 else np.uint16).reshape(len(frames),rows,cols)
    return img, ss
what=sys.argv[1]
if what=="enc":
    for bits in (8,16):
        for rows in (1,3):
            for cols in m.COLS:
                c=m.raster_cases(rows,cols,bits); imgs=np.stack(list(c.values()))
                got=enc(imgs)
                for name,g,x in zip(c,got,imgs):
                    assert g==m.encode_frame(x),(bits,rows,cols,name)
        print("enc ok",bits)
elif what=="dec":
    for bits in (8,16):
        for rows,cols in ((1,1),(2,65),(3,300)):
            c=m.raster_cases(rows,cols,bits); imgs=np.stack(list(c.values()))
            for src in (m.encode_frame, m.libtiff_frame):
                back,ss=dec([src(x) for x in imgs],rows,cols,bits)
                assert not ss.any() and np.array_equal(back,imgs),(bits,rows,cols)
        print("dec ok",bits)
elif what=="tile":
    import importlib.util
    rows, cols = 49,128; TILE=2048
    rng = np.random.default_rng(5)
    def frame8(seg): return struct.pack("<16I", 1, 64, *([0] * 14)) + bytes(seg)
    def prefix(s): return b"" if s == 0 else bytes([128]) if s == 1 else bytes([s - 2]) + rng.integers(0, 256, s - 1, dtype=np.uint8).tobytes()
    def literals(k): return b"".join(bytes([127]) + rng.integers(0, 256, 128, dtype=np.uint8).tobytes() for _ in range(k))
    frames=[]
    for s in (0,1,2,3,64,127,128):
        frames.append(frame8(prefix(s) + literals(49)))
        head = prefix(s) + literals(14); gap = TILE - 1 - len(head)
        head += prefix(min(gap,129))
        if gap>129: head += prefix(gap-129)
        frames.append(frame8(head + bytes([257 - 100, 0x5A]) + literals(49)))
    # short one and hand-built
    frames.append(frame8(literals(10)))
    want=[]
    for f in frames:
        try: want.append(m.decode_frame(f,rows,cols,8))
        except ValueError: want.append(None)
    back,ss=dec(frames,rows,cols,8)
    for i,w in enumerate(want):
        if w is None: assert ss[i]==1,i
        else: assert ss[i]==0 and np.array_equal(back[i],w),i
    print("tile ok")
