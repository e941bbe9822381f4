// Host-only check of the compiled-tree agreement test of the model builder
// (mj_envs_amd/csrc/aw_model_host.h check_tree with the built MData), run by tests/test_tree_check.py:
//   tree_check TABLE [ANCMASK_ROW ANCMASK_BIT]
// builds the device tables of the model table file as aw_create does, optionally flips one bit of
// the built dof_ancmask (the table stage_crb no longer reads, the solver stages still do), runs
// check_tree and prints "build=<rc> tree=<rc> msg=<message>".
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -o tree_check tree_check.cc
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../mj_envs_amd/csrc/aw_model_host.h"

using namespace aw;

template <class T>
struct Zeroed {
  std::unique_ptr<unsigned char[]> mem{new unsigned char[sizeof(T)]()};
  T& get() { return *reinterpret_cast<T*>(mem.get()); }
};

int main(int argc, char** argv) {
  if (argc != 2 && argc != 4) { fprintf(stderr, "usage: tree_check TABLE [ROW BIT]\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
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
  if (!rc_build) {
    if (argc == 4) {
      const int row = atoi(argv[2]), bit = atoi(argv[3]);
      if (row < 0 || row >= MAXV || bit < 0 || bit >= 64) { fprintf(stderr, "row / bit out of range\n"); return 2; }
      md.get().dof_ancmask[row] ^= 1ull << bit;
    }
    rc_tree = check_tree(B, m.get().task_kind, md.get(), msg);
  }
  printf("build=%d tree=%d msg=%s\n", rc_build, rc_tree, msg.c_str());
  return 0;
}
