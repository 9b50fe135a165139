// Host-only pieces of the run-time RCCL binding of csrc/ismpc_group.hip: which copy of librccl a process already maps, and the
// dlopen over a list of candidates.  No HIP and no RCCL types, so that a plain g++ program can run them under the sanitizers
// (tests/helpers/rccl_load_probe.cpp).
#pragma once
#include <dlfcn.h>

#include <cstring>
#include <string>
#include <vector>

namespace ismpc_rccl {

// One line of /proc/self/maps -> the path of the librccl.so it maps, or "" if it maps none.  The path is everything from the first
// '/' (the fields before it hold none; a path may contain blanks), without the newline, trailing blanks and the " (deleted)" the
// kernel appends once the file was unlinked.
inline std::string maps_line_path(const char* line)
{
    if (!line || !std::strstr(line, "librccl.so")) return "";
    const char* s = std::strchr(line, '/');
    if (!s) return "";
    std::string path(s);
    auto rstrip = [&path] { while (!path.empty() && (path.back() == '\n' || path.back() == '\r' || path.back() == ' ' || path.back() == '\t')) path.pop_back(); };
    rstrip();
    static const char deleted[] = " (deleted)";
    const size_t n = sizeof deleted - 1;
    if (path.size() >= n && path.compare(path.size() - n, n, deleted) == 0) { path.erase(path.size() - n); rstrip(); }
    return path;
}

struct Opened {
    void* lib = nullptr;                 // handle of the first candidate that opened, or NULL
    std::string path;                    // that candidate
    std::vector<std::string> errors;     // "<candidate>: <the loader's message>", one per candidate that failed before it
    std::string error_text() const { std::string s; for (const std::string& e : errors) s += e + "; "; return s; }
};

// dlopen(RTLD_NOW | RTLD_LOCAL) of the candidates in order, up to the first that opens.
inline Opened open_first(const std::vector<std::string>& candidates)
{
    Opened o;
    for (const std::string& c : candidates) {
        o.lib = dlopen(c.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (o.lib) { o.path = c; break; }
        const char* e = dlerror();       // once: the call clears the message
        o.errors.push_back(c + ": " + (e ? e : "?"));
    }
    return o;
}

}  // namespace ismpc_rccl
