#include "backend.h"

#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

// FFH_BACKEND_LIB points the driver at another library exporting include/ff_hip.h (the CPU oracle in tests, an A/B build).  It is
// the one environment variable this layer reads, so it is never silent: load_kernel_api() says on stderr which library an
// override selected, and the driver names the kernel library on its THROUGHPUT line whenever it is not the product's own
// (KernelApi::overridden).
static bool g_env_override = false;
std::string default_backend_path() {
  if (const char* e = getenv("FFH_BACKEND_LIB")) { g_env_override = true; return std::string(e); }
  Dl_info info;
  std::string dir = ".";
  if (dladdr((void*)&default_backend_path, &info) && info.dli_fname) {
    std::string p(info.dli_fname);
    size_t k = p.rfind('/');
    if (k != std::string::npos) dir = p.substr(0, k);
  }
  return dir + "/../csrc/libffhip.so";
}

// The rule for an optional extension (a line of FFH_EXTENSIONS in backend.h), stated once: absent is fine (the library loads as before),
// present means complete and of the header's version.  `older` is the one allowance a line may make: a library of that ABI version is taken
// as it is, and the entries whose names begin with one of `may_lack` may be missing from it (they stay null).
namespace {
struct OlderAbi {
  int version = 0;                       // 0: none
  const char* may_lack[4] = {};
};

struct ExtensionLoad {
  void* h;
  const std::string& path;
  const char* label;
  const char* header;
  int expected, got;                     // the header's version, what the library's version symbol returns
  OlderAbi older;

  bool older_abi() const { return older.version && got == older.version; }

  template <class Fn>
  void entry(Fn& slot, const char* name) const {
    slot = reinterpret_cast<Fn>(dlsym(h, name));
    if (slot) return;
    if (older_abi())
      for (const char* p : older.may_lack)
        if (p && !strncmp(name, p, strlen(p))) return;
    fprintf(stderr, "FATAL: %s exports part of include/%s: %s is missing\n", path.c_str(), header, name);
    abort();
  }

  void check_version() const {
    if (got == expected || older_abi()) return;
    fprintf(stderr, "FATAL: %s has %s ABI version %d, expected %d\n", path.c_str(), label, got, expected);
    abort();
  }
};
}  // namespace

const KernelApi* load_kernel_api(const std::string& path_in) {
  static std::map<std::string, KernelApi*>& cache = *new std::map<std::string, KernelApi*>();   // one table per library for the life of the process
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  const std::string path = path_in.empty() ? default_backend_path() : path_in;
  auto it = cache.find(path);
  if (it != cache.end()) return it->second;
  void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
  if (!h) {
    fprintf(stderr, "FATAL: cannot load kernel library %s: %s\n"
                    "       build it with: python -c 'import __graft_entry__ as g; g.build()'\n", path.c_str(), dlerror());
    abort();
  }
  KernelApi* api = new KernelApi();
  api->handle = h;
  api->path = path;
  api->overridden = !path_in.empty() || g_env_override;
#define FFH_LOAD(name)                                                        \
  api->name = reinterpret_cast<decltype(api->name)>(dlsym(h, #name));         \
  if (!api->name) {                                                           \
    fprintf(stderr, "FATAL: %s does not export %s\n", path.c_str(), #name);   \
    abort();                                                                  \
  }
  FFH_API_LIST(FFH_LOAD)
#undef FFH_LOAD
  if (api->ffh_abi_version() != FFH_ABI_VERSION) {
    fprintf(stderr, "FATAL: %s has ABI version %d, expected %d\n", path.c_str(), api->ffh_abi_version(), FFH_ABI_VERSION);
    abort();
  }
  // the optional extensions, in the list's order: the version symbol says whether one is there
#define FFH_LOAD_ENTRY(name) ext.entry(b->name, #name);
#define FFH_LOAD_EXTENSION(field, Struct, LIST, version_symbol, VERSION, label, header, ...)               \
  if (auto version = reinterpret_cast<int (*)(void)>(dlsym(h, #version_symbol))) {                          \
    const ExtensionLoad ext{h, path, label, header, VERSION, version(), {__VA_ARGS__}};                     \
    Struct* b = new Struct();                                                                               \
    LIST(FFH_LOAD_ENTRY)                                                                                    \
    ext.check_version();                                                                                    \
    api->field = b;                                                                                         \
  }
  FFH_EXTENSIONS(FFH_LOAD_EXTENSION)
#undef FFH_LOAD_EXTENSION
#undef FFH_LOAD_ENTRY
  if (path_in.empty() && g_env_override)
    fprintf(stderr, "[DLRM] FFH_BACKEND_LIB: kernel library %s (%s)\n", path.c_str(), api->ffh_backend_name());
  cache[path] = api;
  return api;
}
