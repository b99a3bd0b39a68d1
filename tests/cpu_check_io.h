// File plumbing shared by the host check programs (tests/cpu_*_check.cpp) that read a binary case file and write a binary
// result file: open or leave with the program's own exit code, read n elements into an exact-size vector, write n elements.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace check_io {

inline FILE* open_or_exit(const char* path, const char* mode, int code) {
  FILE* f = fopen(path, mode);
  if (!f) exit(code);
  return f;
}

// v becomes exactly n elements (the sanitizer sees a read past the last one); false on a short file
template <typename T>
bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// nothing for n == 0: an empty vector's data() may be null, which fwrite must not be handed
template <typename T>
bool write_vec(FILE* f, const T* p, size_t n) {
  return n == 0 || fwrite(p, sizeof(T), n, f) == n;
}

template <typename T>
bool write_vec(FILE* f, const std::vector<T>& v) { return write_vec(f, v.data(), v.size()); }

}  // namespace check_io
