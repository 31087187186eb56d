#!/usr/bin/env python3
"""Build libfthe.so (the MI355X batch Paillier engine) in-tree.

Steps
  1. generate the hand-scheduled Montgomery program kernels (gen_montprog.py) for each limb count,
     the P-adic exponentiation kernels (gen_padic.py) and the n-adic public-encrypt kernel
     (gen_nadic.py), assemble + link them into gfx950 code objects;
  2. embed the code objects into gen/montprog_blobs.h;
  3. hipcc the host/C-ABI and glue kernels into fedtree_amd/libfthe.so.
GMP (host-side key set-up only) is the system libgmp.so.10; headers from
/opt/conda/include are searched after the system ones.
"""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
GEN = os.path.join(CSRC, "gen")
LLVM = "/opt/rocm/lib/llvm/bin"
ARCH = "gfx950"
VARIANTS = ((37, 28, 12, False), (74, 28, 12, False), (152, 27, 4, True), (80, 27, 4, True))   # (limbs, radix bits, outer unroll, four lanes per ciphertext)
DEFAULT_OUT = os.path.join(HERE, "libfthe.so")
OUT = os.path.abspath(os.environ.get("FTHE_BUILD_OUT") or DEFAULT_OUT)   # A/B builds elsewhere


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        raise SystemExit(r.returncode)
    return r


def build_kernels():
    os.makedirs(GEN, exist_ok=True)
    sys.path.insert(0, CSRC)
    # A/B generator switches (FTHE_GEN_*: tools/build_m37_ab.sh, the FTHE_GEN_NADIC_AB library A/Bs; some give
    # wrong results by design, e.g. FTHE_GEN_NADIC_AB=noest) reach only a library built elsewhere
    # (FTHE_BUILD_OUT), never the in-tree libfthe.so.  Removed before the generators are imported: some read
    # their switches at import time.  gen_padic_mfma, gen_addb and gen_nadicb take theirs as arguments: read below,
    # after the scrub.
    if OUT == DEFAULT_OUT:
        for k in sorted(k for k in os.environ if k.startswith("FTHE_GEN_")):
            os.environ.pop(k)
            sys.stderr.write(f"build.py: ignoring {k} (A/B generator switch) for the in-tree library\n")
    m37_ab = os.environ.get("FTHE_GEN_M37_AB", "")
    m37k_ab = os.environ.get("FTHE_GEN_M37K_AB", m37_ab)      # fthe_padic_m37k also knows switches of its own
    addb_dbg = os.environ.get("FTHE_GEN_ADDB_DBG", "")
    nadicb_dbg = os.environ.get("FTHE_GEN_NADICB_DBG", "")
    import gen_montprog  # noqa: E402
    import gen_padic  # noqa: E402
    import gen_nadic  # noqa: E402
    import gen_padic_mfma  # noqa: E402
    import gen_addb  # noqa: E402
    import gen_nadicb  # noqa: E402
    nadicb_waves = int(os.environ.get("FTHE_GEN_NADICB_WAVES", gen_nadicb.WAVES))     # timing builds only
    for lay_name, new_lay in (("addb_layout.h", gen_addb.layout_header()),
                              ("nadicb_layout.h", gen_nadicb.layout_header(nadicb_waves))):
        lay = os.path.join(GEN, lay_name)
        if not os.path.exists(lay) or open(lay).read() != new_lay:
            with open(lay, "w") as f:
                f.write(new_lay)
    blobs = []
    # the P-adic exponentiation kernels (digits of K = 37 / 19 limbs) are registered as pseudo-variants 1000 + K
    kernels = [(S, f"fthe_montprog_s{S}", f"montprog_s{S}",
                (lambda S=S, B=B, U=U, quad=quad, n=f"fthe_montprog_s{S}":
                 (gen_montprog.gen_quad if quad else gen_montprog.gen)(S, B, U, n)))
               for S, B, U, quad in VARIANTS]
    for K in (37, 19):
        kernels.append((1000 + K, f"fthe_padic_k{K}", f"padic_k{K}",
                        lambda K=K: gen_padic.gen_padic(K, 28, f"fthe_padic_k{K}")))
    # the K = 37 P-adic kernel with matrix-core Barrett reductions: pseudo-variant 1137; its four-tile body (product 2
    # of the reductions without its fifth M-tile): 1237; the four-tile body on product 1's operand shifted by 8 bytes
    # (15 instead of 19 product-1 tiles): 1337; with product 1 fed q1's limbs as they lie (no repack): 1437; that one
    # with MUL's cross term by Karatsuba: 1537
    for S, body in ((1137, "m37"), (1237, "m37t"), (1337, "m37s"), (1437, "m37l"), (1537, "m37k")):
        kernels.append((S, f"fthe_padic_{body}", f"padic_{body}",
                        lambda body=body: gen_padic_mfma.gen_body(body, m37_ab if body != "m37k" else m37k_ab)))
    # the n-adic four-lane kernel of the public-key encrypt (base-n digits of 76 limbs): pseudo-variant 2076
    kernels.append((2076, "fthe_nadic_q76", "nadic_q76", lambda: gen_nadic.gen_nadic(76, 27, "fthe_nadic_q76")))
    # its Montgomery form (LSB-first reductions, no quotient estimates): pseudo-variant 2176
    kernels.append((2176, "fthe_nadic_m76", "nadic_m76",
                    lambda: gen_nadic.gen_nadic(76, 27, "fthe_nadic_m76", mont=True)))
    # its matrix-core Barrett form (products on the VALU, both Barrett reductions by n on i8 MFMA): 2276
    kernels.append((2276, "fthe_nadic_b76", "nadic_b76",
                    lambda: gen_nadicb.gen_nadicb("fthe_nadic_b76", nadicb_waves, nadicb_dbg)))
    # the P-2048 ciphertext add with a matrix-core Barrett reduction (not an op-program kernel): blob 3152
    kernels.append((3152, "fthe_addb_q152", "addb_q152", lambda: gen_addb.gen_addb("fthe_addb_q152", addb_dbg)))
    # its paired entry point (x y and x y2 in one launch, x unpacked once: the batched inverse's down step): blob 3153
    kernels.append((3153, "fthe_addb_pair", "addb_pair", lambda: gen_addb.gen_addb("fthe_addb_pair", "pair")))
    for S, name, stem, make in kernels:
        asm = os.path.join(GEN, f"{stem}.s")
        src = make()
        old = open(asm).read() if os.path.exists(asm) else None
        if old != src:
            with open(asm, "w") as f:
                f.write(src)
        obj = os.path.join(GEN, f"{stem}.o")
        hsaco = os.path.join(GEN, f"{stem}.hsaco")
        run([f"{LLVM}/clang", "-x", "assembler", "-target", "amdgcn-amd-amdhsa", f"-mcpu={ARCH}",
             "-c", asm, "-o", obj])
        run([f"{LLVM}/ld.lld", "-shared", obj, "-o", hsaco])
        blobs.append((S, open(hsaco, "rb").read()))
    hdr = ["// generated by fedtree_amd/build.py -- gfx950 code objects of the montprog kernels",
           "#pragma once", "#include <cstddef>", ""]
    for S, b in blobs:
        hdr.append(f"alignas(64) static const unsigned char fthe_blob_s{S}[{len(b)}] = {{")
        for i in range(0, len(b), 24):
            hdr.append("  " + ",".join(str(x) for x in b[i:i + 24]) + ",")
        hdr.append("};")
    hdr.append("static inline const unsigned char *fthe_montprog_blob(int S) {")
    for S, _ in blobs:
        hdr.append(f"  if (S == {S}) return fthe_blob_s{S};")
    hdr.append("  return nullptr;")
    hdr.append("}")
    path = os.path.join(GEN, "montprog_blobs.h")
    new = "\n".join(hdr) + "\n"
    if not os.path.exists(path) or open(path).read() != new:
        with open(path, "w") as f:
            f.write(new)


def build_lib():
    srcs = [os.path.join(CSRC, "fthe.hip"), os.path.join(CSRC, "fthe_glue.hip"), os.path.join(CSRC, "fthe_hist.hip"),
            os.path.join(CSRC, "fthe_dec.hip"), os.path.join(CSRC, "fthe_wire.cpp")]
    deps = srcs + [os.path.join(CSRC, f) for f in ("bn_host.hpp", "fthe_glue.h", "padic_tiles.hpp", "barrett_image.hpp",
                                                    "addb_image.hpp", "nadicb_image.hpp", "group_commit.hpp")] + \
        [os.path.join(GEN, "montprog_blobs.h"), os.path.join(GEN, "addb_layout.h"), os.path.join(GEN, "nadicb_layout.h"),
         os.path.join(HERE, "..", "include", "fthe.h")]
    cmd = ["/opt/rocm/bin/hipcc", f"--offload-arch={ARCH}", "-O3", "-fPIC", "-shared", "-std=c++17",
           "-idirafter", "/opt/conda/include", "-Wno-unused-result",
           *(["-DFTHE_STAMP_HOOK"] if OUT != DEFAULT_OUT else []),   # timing hook: A/B libraries only
           *srcs, "-l:libgmp.so.10", "-o", OUT + ".tmp"]
    # content hash of every input and of the command, not mtimes: a snapshot copied to another machine keeps no
    # meaningful mtimes, so the library is reused only when it was built from exactly these bytes
    h = hashlib.sha256(" ".join(cmd[:-2]).encode())
    for d in deps:
        with open(d, "rb") as f:
            h.update(os.path.basename(d).encode() + b"\0" + f.read())
    digest = h.hexdigest()
    stamp = OUT + ".sha256"
    if os.path.exists(OUT) and os.path.exists(stamp) and open(stamp).read().strip() == digest:
        return
    run(cmd)
    os.replace(OUT + ".tmp", OUT)
    with open(stamp, "w") as f:
        f.write(digest + "\n")


def main():
    build_kernels()
    build_lib()
    print(OUT)


if __name__ == "__main__":
    main()
