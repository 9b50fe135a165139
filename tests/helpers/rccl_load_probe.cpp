// Sanitizer driver for the host-only RCCL loader (csrc/ismpc_rccl_load.hpp): g++ -fsanitize=address,undefined, CPU only.
//   usage: rccl_load_probe <a library that exists, e.g. libm.so.6>
#include <cstdio>
#include <string>
#include <vector>

#include "ismpc_rccl_load.hpp"

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return 1; } } while (0)

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage\n"); return 2; }
    const std::string missing_a = "/nonexistent/librccl_probe_a.so", missing_b = "librccl_probe_b_not_there.so.9";

    // ---- every candidate is missing: no handle, one message per candidate, each the loader's own (it names the file)
    {
        const ismpc_rccl::Opened o = ismpc_rccl::open_first({missing_a, missing_b});
        CHECK(o.lib == nullptr && o.path.empty(), "a handle from nothing: %s", o.path.c_str());
        CHECK(o.errors.size() == 2, "%zu error texts for 2 candidates", o.errors.size());
        const std::string cand[2] = {missing_a, missing_b};
        for (int k = 0; k < 2; ++k) {
            const std::string& e = o.errors[k];
            CHECK(e.compare(0, cand[k].size() + 2, cand[k] + ": ") == 0, "error %d does not start with its candidate: %s", k, e.c_str());
            const std::string msg = e.substr(cand[k].size() + 2);
            CHECK(msg != "?" && msg.size() > 8, "error %d carries no loader message: %s", k, e.c_str());
            CHECK(msg.find(cand[k]) != std::string::npos, "the loader's message names the file it missed: %s", e.c_str());
            std::printf("missing[%d] %s\n", k, e.c_str());
        }
        const std::string all = o.error_text();
        CHECK(all.find(missing_a) != std::string::npos && all.find(missing_b) != std::string::npos && all.find(": ?;") == std::string::npos, "joined text: %s", all.c_str());
        const ismpc_rccl::Opened none = ismpc_rccl::open_first({});
        CHECK(none.lib == nullptr && none.errors.empty() && none.error_text().empty(), "empty list");
    }
    // ---- the first is missing, the second exists: the second is opened and reported
    {
        const ismpc_rccl::Opened o = ismpc_rccl::open_first({missing_a, argv[1], missing_b});
        CHECK(o.lib != nullptr, "%s did not open: %s", argv[1], o.error_text().c_str());
        CHECK(o.path == argv[1], "path %s", o.path.c_str());
        CHECK(o.errors.size() == 1 && o.errors[0].compare(0, missing_a.size(), missing_a) == 0, "one failure before it, %zu recorded", o.errors.size());
        dlclose(o.lib);
        std::printf("opened %s\n", o.path.c_str());
    }
    // ---- /proc/self/maps lines
    {
        struct { const char* line; const char* want; } cases[] = {
            {"7f3a1c000000-7f3a1c9b2000 r-xp 00000000 08:01 1316407                    /opt/rocm-7.0.0/lib/librccl.so.1.0.70000\n", "/opt/rocm-7.0.0/lib/librccl.so.1.0.70000"},
            {"7f3a1c000000-7f3a1c9b2000 r-xp 00000000 08:01 1316407                    /tmp/x/librccl.so (deleted)\n", "/tmp/x/librccl.so"},
            {"7f3a1c000000-7f3a1c9b2000 r-xp 00000000 08:01 1316407                    /usr/lib/libamdhip64.so.7\n", ""},
            {"7f3a1c000000-7f3a1c9b2000 rw-p 00000000 00:00 0                          [anon: librccl.so]\n", ""},
            {"7f3a1c000000-7f3a1c9b2000 r--p 00000000 08:01 77   /home/some user/site packages/torch/lib/librccl.so  \n", "/home/some user/site packages/torch/lib/librccl.so"},
            {"7f3a1c000000-7f3a1c9b2000 r--p 00000000 08:01 77   /home/some user/librccl.so (deleted)", "/home/some user/librccl.so"},
            {"", ""},
        };
        for (auto& c : cases) {
            const std::string got = ismpc_rccl::maps_line_path(c.line);
            CHECK(got == c.want, "maps line [%s] -> [%s], expected [%s]", c.line, got.c_str(), c.want);
        }
        CHECK(ismpc_rccl::maps_line_path(nullptr).empty(), "null line");
        std::printf("maps %zu lines\n", sizeof cases / sizeof cases[0]);
    }
    std::printf("OK rccl_load_probe\n");
    return 0;
}
