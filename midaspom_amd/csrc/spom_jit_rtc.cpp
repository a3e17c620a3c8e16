// midaspom_amd/csrc/spom_jit_rtc.cpp -- problem-specialised forward kernel:
// compiling its generated source (spom_jit.cpp) with hipRTC.
//
// Code objects are cached in memory and on disk, keyed by the FNV-1a hash of
// the generated source, the compile options and the hipRTC version; a cached
// file that is not a gfx950 code object, or that the runtime refuses to load
// (spom_engine.hip jit_load), is rebuilt.  hipRTC itself (and the compiler
// library it brings in) is loaded with dlopen on the first cache miss only: a
// run whose code objects are all cached never maps it (the drop-in CLI's
// start-up, main_MIDASPOM.c:326-332).
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <hip/hiprtc.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "spom_jit.h"

// The HIP runtime's version query, as a weak reference: libmidaspom.so links
// the runtime, so it resolves there as ever; a host-only program that links
// this object without the runtime (plan_check, whose planner object refers to
// mdp_jit_compile in jit_build but never compiles) gets a null address
// instead of an undefined symbol.
extern "C" hipError_t hipRuntimeGetVersion(int *) __attribute__((weak));

namespace {

uint64_t fnv1a(const std::string &s)
{
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : s) {
        h ^= c;
        h *= 1099511628211ull;
    }
    return h;
}

// The disk cache: MDP_JIT_CACHE, else ~/.cache/midaspom_jit, else (no
// HOME) a per-user /tmp/midaspom_jit-<uid>.  The directory is created 0700
// and used only while it is owned by this user and writable by nobody else
// (cache_dir_private): a code object found there is loaded into the GPU, so
// a directory another user can write to is not a cache.
std::string cache_dir()
{
    if (const char *d = getenv("MDP_JIT_CACHE")) return d;
    if (const char *h = getenv("HOME")) return std::string(h) + "/.cache/midaspom_jit";
    return "/tmp/midaspom_jit-" + std::to_string((long)geteuid());
}

bool cache_dir_private(const std::string &dir)
{
    struct stat st;
    if (lstat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return false;
    return st.st_uid == geteuid() && (st.st_mode & (S_IWGRP | S_IWOTH)) == 0;
}

// create the cache directory (and its parent, e.g. ~/.cache) if missing
void make_cache_dir(const std::string &dir)
{
    const size_t sl = dir.find_last_of('/');
    if (sl != std::string::npos && sl > 0) mkdir(dir.substr(0, sl).c_str(), 0755);
    mkdir(dir.c_str(), 0700);
}

bool read_file(const std::string &path, std::vector<char> &out)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    rewind(f);
    if (n <= 0) {
        fclose(f);
        return false;
    }
    out.resize((size_t)n);
    bool ok = fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

void write_file(const std::string &dir, const std::string &path, const std::vector<char> &data)
{
    make_cache_dir(dir);
    if (!cache_dir_private(dir)) return;
    static std::atomic<unsigned> seq{0};  // threads of one process write distinct temporaries
    std::string tmp = path + ".tmp" + std::to_string((long)getpid()) + "." + std::to_string(seq++);
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return;
    const bool ok = fwrite(data.data(), 1, data.size(), f) == data.size();
    fclose(f);
    if (ok) rename(tmp.c_str(), path.c_str());
    else remove(tmp.c_str());
}

std::mutex g_mu;
std::map<uint64_t, std::vector<char>> g_code;  // in-process code-object cache

// hipRTC entry points, resolved from libhiprtc on first use
struct RtcApi {
    bool ok = false;
    std::string err;
    decltype(&hiprtcCreateProgram) create = nullptr;
    decltype(&hiprtcCompileProgram) compile = nullptr;
    decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
    decltype(&hiprtcGetProgramLog) get_log = nullptr;
    decltype(&hiprtcGetCodeSize) code_size = nullptr;
    decltype(&hiprtcGetCode) get_code = nullptr;
    decltype(&hiprtcDestroyProgram) destroy = nullptr;
    decltype(&hiprtcGetErrorString) errstr = nullptr;
};

const RtcApi &rtc()
{
    static RtcApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void *h = nullptr;
        for (const char *name : {"libhiprtc.so.7", "libhiprtc.so"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) {
            const char *e = dlerror();
            api.err = std::string("cannot load libhiprtc: ") + (e ? e : "?");
            return;
        }
        bool all = true;
        auto sym = [&](auto &fp, const char *name) {
            fp = reinterpret_cast<std::remove_reference_t<decltype(fp)>>(dlsym(h, name));
            all = all && fp;
        };
        sym(api.create, "hiprtcCreateProgram");
        sym(api.compile, "hiprtcCompileProgram");
        sym(api.log_size, "hiprtcGetProgramLogSize");
        sym(api.get_log, "hiprtcGetProgramLog");
        sym(api.code_size, "hiprtcGetCodeSize");
        sym(api.get_code, "hiprtcGetCode");
        sym(api.destroy, "hiprtcDestroyProgram");
        sym(api.errstr, "hiprtcGetErrorString");
        api.ok = all;
        if (!all) api.err = "libhiprtc lacks an entry point";
    });
    return api;
}

// (kernel-argument preload: the first 14 argument SGPRs -- all that
// mdp_fwd_jit's front reads -- arrive with the wave instead of through a
// scalar load; the compiler's compatibility prologue loads them where the
// firmware does not preload)
#ifndef MDP_JIT_NO_PRELOAD
const char *const kJitOpts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-kernarg-preload-count=14"};
#else
const char *const kJitOpts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
#endif
constexpr int kJitNOpts = (int)(sizeof kJitOpts / sizeof kJitOpts[0]);
constexpr int kJitCacheFormat = 4;  // bump when the cache key or file layout changes

// The compiler's file identity without loading it: the resolved path, size
// and mtime of libhiprtc and libamd_comgr next to the HIP runtime this
// library runs on (located by dladdr), plus LD_LIBRARY_PATH, which can make
// the dlopen in hiprtc_api() find another libhiprtc.  A comgr / hipRTC
// hotfix without a runtime version bump then changes the key.
const std::string &toolchain_identity()
{
    static std::once_flag once;
    static std::string id;
    std::call_once(once, [] {
        Dl_info di{};
        std::string dir;
        if (hipRuntimeGetVersion && dladdr((const void *)&hipRuntimeGetVersion, &di) && di.dli_fname) {
            dir = di.dli_fname;
            const size_t sl = dir.rfind('/');
            dir = sl == std::string::npos ? std::string(".") : dir.substr(0, sl);
        }
        for (const char *lib : {"libhiprtc.so.7", "libamd_comgr.so.3"}) {
            const std::string p = dir + "/" + lib;
            struct stat st{};
            char real[4096];
            id += lib;
            if (!dir.empty() && stat(p.c_str(), &st) == 0) {
                id += ' ';
                id += realpath(p.c_str(), real) ? real : p.c_str();
                id += ' ' + std::to_string((long long)st.st_size) + ' ' + std::to_string((long long)st.st_mtime);
            }
            id += ';';
        }
        if (const char *lp = getenv("LD_LIBRARY_PATH")) (id += " ldpath ") += lp;
    });
    return id;
}

// Cache key: the generated source, the compile options, the ROCm release
// (the HIP runtime's version, which hipRTC ships with -- asking hipRTC itself
// would load it on every run), the compiler libraries' file identity and the
// cache format.  A code object built by another toolchain or with other
// options therefore lands under another name.
uint64_t jit_key(const std::string &src)
{
    int rt = 0;
    if (hipRuntimeGetVersion) (void)hipRuntimeGetVersion(&rt);
    std::string k = src;
    k += '\0';
    for (const char *o : kJitOpts) (k += o) += ' ';
    k += "hip " + std::to_string(rt) + " headers " + std::to_string(HIP_VERSION) + " format " +
         std::to_string(kJitCacheFormat) + " tools " + toolchain_identity();
    return fnv1a(k);
}

// Cache files are the code object followed by a 16-byte trailer: "MDPJ", the
// format, and the 64-bit key it was compiled for.  A file whose trailer does
// not name this key (a stale or corrupted file, another format, another
// key's object under this name) is a miss.  The trailer is a staleness and
// corruption check, not an authentication: the key is also the file name.
// What keeps other users' objects out is the directory check
// (cache_dir_private).
constexpr char kTrailerMagic[4] = {'M', 'D', 'P', 'J'};

void add_trailer(std::vector<char> &c, uint64_t key)
{
    const uint32_t fmt = kJitCacheFormat;
    c.insert(c.end(), kTrailerMagic, kTrailerMagic + 4);
    c.insert(c.end(), (const char *)&fmt, (const char *)&fmt + 4);
    c.insert(c.end(), (const char *)&key, (const char *)&key + 8);
}

bool strip_trailer(std::vector<char> &c, uint64_t key)
{
    if (c.size() < 16) return false;
    const char *t = c.data() + c.size() - 16;
    uint32_t fmt;
    uint64_t k;
    memcpy(&fmt, t + 4, 4);
    memcpy(&k, t + 8, 8);
    if (memcmp(t, kTrailerMagic, 4) != 0 || fmt != (uint32_t)kJitCacheFormat || k != key) return false;
    c.resize(c.size() - 16);
    return true;
}

// ... and what precedes it must be an AMDGPU ELF code object for gfx950
// (e_machine EM_AMDGPU = 224, EF_AMDGPU_MACH = 0x04f).
bool plausible_code_object(const std::vector<char> &c)
{
    if (c.size() < 64 || memcmp(c.data(), "\x7f" "ELF", 4) != 0) return false;
    uint16_t machine;
    uint32_t flags;
    memcpy(&machine, c.data() + 18, sizeof machine);
    memcpy(&flags, c.data() + 48, sizeof flags);
    return machine == 224 && (flags & 0xffu) == 0x4fu;
}

}  // namespace

int mdp_jit_compile(const std::string &src, std::vector<char> &code, std::string &log, bool fresh)
{
    const uint64_t key = jit_key(src);
    if (!fresh) {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_code.find(key);
        if (it != g_code.end()) {
            code = it->second;
            return 0;
        }
    }
    char name[64];
    snprintf(name, sizeof name, "fwd_%016llx.co", (unsigned long long)key);
    const std::string dir = cache_dir();
    const std::string path = dir + "/" + name;
    if (!fresh && !getenv("MDP_JIT_NOCACHE") && cache_dir_private(dir) && read_file(path, code) &&
        strip_trailer(code, key) && plausible_code_object(code)) {
        std::lock_guard<std::mutex> lk(g_mu);
        g_code[key] = code;
        return 0;
    }
    const RtcApi &R = rtc();
    if (!R.ok) {
        log = R.err;
        return -1;
    }
    hiprtcProgram prog;
    if (R.create(&prog, src.c_str(), "mdp_fwd_jit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        log = "hiprtcCreateProgram failed";
        return -1;
    }
    const hiprtcResult r = R.compile(prog, kJitNOpts, kJitOpts);
    size_t ls = 0;
    R.log_size(prog, &ls);
    if (ls > 1) {
        std::vector<char> lb(ls + 1, 0);
        R.get_log(prog, lb.data());
        log = lb.data();
    }
    if (r != HIPRTC_SUCCESS) {
        R.destroy(&prog);
        if (log.empty()) log = R.errstr(r);
        return -1;
    }
    size_t cs = 0;
    R.code_size(prog, &cs);
    code.resize(cs);
    R.get_code(prog, code.data());
    R.destroy(&prog);
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_code[key] = code;
    }
    if (!getenv("MDP_JIT_NOCACHE")) {
        std::vector<char> file = code;
        add_trailer(file, key);
        write_file(dir, path, file);
    }
    return 0;
}
