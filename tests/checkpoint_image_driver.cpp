// checkpoint_image_driver.cpp — a stand-alone program over csrc/coflux_checkpoint_image.cpp alone (no HIP, no libcoflux):
// it reads every file named on its command line as a checkpoint image, copies it into a heap block of exactly its size (so
// that a read one byte beyond the image is a read beyond an allocation) and prints one line per file,
//     <path>\tOK   |   <path>\tREFUSED\t<message>
// tests/test_checkpoint_cpu.py builds it with -fsanitize=address,undefined and replays its designed corrupt images.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "coflux_checkpoint_image.hpp"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<unsigned char> all;
        unsigned char buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + n);
        std::fclose(f);
        unsigned char* exact = static_cast<unsigned char*>(std::malloc(all.size() ? all.size() : 1));
        if (!all.empty()) std::memcpy(exact, all.data(), all.size());
        char msg[512] = "";
        cfck::Header H{};
        const int rc = cfck::verify(exact, all.size(), &H, msg, sizeof msg);
        // the hash of the whole file as well: every byte is read, the short last word included
        const unsigned long long h = cfck::hash_bytes(exact, all.size());
        if (rc == 0) std::printf("%s\tOK\t%016llx\n", argv[a], h);
        else std::printf("%s\tREFUSED\t%s\n", argv[a], msg);
        std::free(exact);
    }
    return 0;
}
