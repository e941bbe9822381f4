// Host-only check of the model builder (mj_envs_amd/csrc/aw_model_host.h), run by
// tests/test_model_build.py: for every model table file named on the command line, build the device
// tables into zero-filled blocks exactly as aw_create does, and print one line with the return
// codes, the message, the block sizes and the 64-bit FNV-1a digest of each block's bytes.
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -o model_build_check model_build_check.cc
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../mj_envs_amd/csrc/aw_model_host.h"

using namespace aw;

static unsigned long long fnv1a(const void* p, size_t n) {
  unsigned long long h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  return h;
}

// zero-filled storage for a T (the structs hold padding: the digest covers every byte)
template <class T>
struct Zeroed {
  std::unique_ptr<unsigned char[]> mem{new unsigned char[sizeof(T)]()};
  T& get() { return *reinterpret_cast<T*>(mem.get()); }
};

static int run(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  std::vector<unsigned char> table;
  unsigned char buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) table.insert(table.end(), buf, buf + k);
  fclose(f);

  Zeroed<DModel> m;
  Zeroed<MData> md;
  Zeroed<SensTab> sens;
  Zeroed<DataTab> data;
  Blob B{table.data(), table.size()};
  std::string msg;
  int rc_build = build_model(B, m.get(), md.get(), sens.get(), data.get(), msg);
  int rc_tree = 0;
  if (!rc_build) rc_tree = check_tree(B, m.get().task_kind, msg);
  printf("build=%d tree=%d sizeof_DModel=%zu sizeof_MData=%zu DModel=%016llx MData=%016llx "
         "SensTab=%016llx DataTab=%016llx msg=%s\n",
         rc_build, rc_tree, sizeof(DModel), sizeof(MData), fnv1a(&m.get(), sizeof(DModel)),
         fnv1a(&md.get(), sizeof(MData)), fnv1a(&sens.get(), sizeof(SensTab)), fnv1a(&data.get(), sizeof(DataTab)),
         msg.c_str());
  return 0;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; i++)
    if (int rc = run(argv[i])) return rc;
  return 0;
}
