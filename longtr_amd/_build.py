"""How libltr_gpu.so is built: the sources, the flags, build() and the id of what it was built from (source_id)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.environ.get("LTR_GPU_LIB") or os.path.join(CSRC, "libltr_gpu.so")   # override: A/B builds only
KERNEL_TUS = ["ltr_k_one.hip", "ltr_k_pack.hip", "ltr_k_plan.hip", "ltr_k_wg.hip", "ltr_k_wgt.hip", "ltr_k_exact.hip", "ltr_k_family.hip"]      # one family of DP kernels each
PLAN_UNITS = ["ltr_plan_rules.cpp", "ltr_plan_sort.cpp", "ltr_plan_families.cpp", "ltr_plan_describe.cpp", "ltr_plan_schedule.cpp", "ltr_plan_hooks.cpp"]      # host-side planning (csrc/ltr_plan.h)
SOURCES = ["ltr_ctx.hip", "ltr_plan_build.hip", "ltr_plan_run.hip", "ltr_posterior.hip", "ltr_plan_genotype.hip", "ltr_plan_fields.hip"] + KERNEL_TUS + ["ltr_short.hip", "ltr_short_batch.cpp", "ltr_nw.hip"] + PLAN_UNITS + ["ltr_host.cpp", "ltr_hap_aln.cpp", "ltr_genotype.cpp", "ltr_vcf.cpp", "ltr_prep.cpp", "ltr_io.cpp", "ltr_bam.cpp", "ltr_vcf_in.cpp", "ltr_editdist.hip", "ltr_poa.hip", "ltr_cluster.cpp"]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-honor-nans", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wall"]
PUBLIC_HEADERS = ["ltr_gpu.h", "ltr_gpu_ploidy.h"]           # include/: what the sources are built against (ltr_filter.h and ltr_snp.h are their own libraries')
LINK_LIBS = ["-lz"]                                         # BGZF blocks (ltr_bgzf.h: BAM, VCF writer, tabix-indexed VCF input)
OBJ_DIR = os.path.join(CSRC, "build")
# The read filter (include/ltr_filter.h) is a host library of its own: libltr_gpu.so, its sources and its source_id stay what they are.
FILTER_SRC = os.path.join(HERE, "filter", "ltr_filter.cpp")
FILTER_LIB_PATH = os.path.join(HERE, "filter", "libltr_filter.so")
FILTER_FLAGS = ["-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall"]
# So are the phasing priors from a phased SNP VCF (include/ltr_snp.h), with the filter's flags.
SNP_SRC = os.path.join(HERE, "snp", "ltr_snp.cpp")
SNP_LIB_PATH = os.path.join(HERE, "snp", "libltr_snp.so")


def build(force=False, extra_flags=()):
    """hipcc cross-compiles for gfx950 without a GPU; the .so stays in-tree.  Every source is its own
    translation unit (objects under csrc/build/, rebuilt when the source or any header is newer), compiled
    side by side on the host cores, then linked."""
    import glob
    from concurrent.futures import ThreadPoolExecutor
    hdrs = glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hpp")) + [os.path.join(HERE, "..", "include", h) for h in PUBLIC_HEADERS]
    hdr_time = max(os.path.getmtime(h) for h in hdrs)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ_DIR, exist_ok=True)
    flags = [f for f in HIPCC_FLAGS if f != "-shared"] + list(extra_flags)
    stamp = os.path.join(OBJ_DIR, "flags.txt")
    if not os.path.exists(stamp) or open(stamp).read() != " ".join(flags):
        force = True
    jobs = []
    for s in SOURCES:
        src, obj = os.path.join(CSRC, s), os.path.join(OBJ_DIR, s + ".o")
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), hdr_time):
            jobs.append([hipcc] + flags + ["-c", src, "-o", obj])
    objs = [os.path.join(OBJ_DIR, s + ".o") for s in SOURCES]
    build_filter(hipcc, force)
    build_snp(hipcc, force)
    if not jobs and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(o) for o in objs):
        return LIB_PATH
    with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), os.cpu_count() or 1))) as ex:
        for r in ex.map(lambda cmd: subprocess.run(cmd), jobs):
            if r.returncode != 0:
                raise subprocess.CalledProcessError(r.returncode, r.args)
    open(stamp, "w").write(" ".join(flags))
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + objs + LINK_LIBS + ["-o", LIB_PATH], check=True)
    return LIB_PATH


def build_filter(compiler=None, force=False):
    """libltr_filter.so from filter/ltr_filter.cpp: host code only, one translation unit, no device pass."""
    compiler = compiler or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    deps = [FILTER_SRC, os.path.join(HERE, "..", "include", "ltr_filter.h")]
    if force or not os.path.exists(FILTER_LIB_PATH) or os.path.getmtime(FILTER_LIB_PATH) < max(os.path.getmtime(d) for d in deps):
        subprocess.run([compiler] + FILTER_FLAGS + [FILTER_SRC, "-o", FILTER_LIB_PATH], check=True)
    return FILTER_LIB_PATH


def build_snp(compiler=None, force=False):
    """libltr_snp.so from snp/ltr_snp.cpp: host code only, one translation unit, no device pass."""
    compiler = compiler or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    deps = [SNP_SRC, os.path.join(HERE, "..", "include", "ltr_snp.h")]
    if force or not os.path.exists(SNP_LIB_PATH) or os.path.getmtime(SNP_LIB_PATH) < max(os.path.getmtime(d) for d in deps):
        subprocess.run([compiler] + FILTER_FLAGS + [SNP_SRC, "-o", SNP_LIB_PATH], check=True)
    return SNP_LIB_PATH


def source_id():
    """Build-path-independent id of the library: SHA-256 (16 hex digits) over the compile flags and the bytes of every source and
    header the .so is built from, in name order.  The .so's own hash changes with the directory it was built in (paths in its
    debug / assert strings); committed counter summaries (profiles/) are matched to a run by THIS id."""
    import glob
    import hashlib
    h = hashlib.sha256(" ".join(HIPCC_FLAGS).encode())
    files = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(CSRC, "*.hip"))
                   + glob.glob(os.path.join(CSRC, "*.cpp")) + [os.path.join(HERE, "..", "include", h) for h in PUBLIC_HEADERS], key=os.path.basename)
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]
