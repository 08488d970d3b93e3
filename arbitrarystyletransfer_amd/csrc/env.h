// The one reader of the AST_* environment switches that remain (DESIGN.md lists them). Each use is
//   static const int x = ast_env::get("AST_...", dflt);
// inside the function that dispatches on it: read once per process, at first use.
#pragma once
#include <cstdlib>

namespace ast_env {
inline int get(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
}  // namespace ast_env
