// dbow2_ref: the reference's own Thirdparty/DBoW2, driven from the command line, as the pin of this project's vocabulary
// path (tests/test_dbow2_reference.py).  This file is ours; the DBoW2 headers and sources come from the reference checkout at
// compile time only (oracle/Makefile, target `ref`, with oracle/ref_shim standing in for OpenCV) and the binary lands in
// oracle/_ref/, which is never committed.
//
//   dbow2_ref transform voc.txt desc.bin levelsup
//       loadFromTextFile(voc.txt); transform(features, BowVector, FeatureVector, levelsup) on the n x 32 bytes of desc.bin.
//       Prints "nBow nFv nWords", then nBow lines "word %a", then nFv lines "node count idx...".
//   dbow2_ref resave in.txt out.txt
//       loadFromTextFile(in.txt); saveToTextFile(out.txt).
//   dbow2_ref distance pairs.bin
//       FORB::distance of every 64-byte pair (a then b), one integer per line.
//   dbow2_ref randomint seed d0 d1 ...
//       DUtils::Random::SeedRandOnce(seed), then RandomInt(0, d_i - 1) for every d_i, one integer per line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "DBoW2/DUtils/Random.h"
#include "DBoW2/FORB.h"
#include "DBoW2/TemplatedVocabulary.h"

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> Vocabulary;

static bool slurp(const char* path, std::vector<unsigned char>& out)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

static cv::Mat row32(const unsigned char* p)
{
    cv::Mat m(1, 32, CV_8U);
    std::memcpy(m.data, p, 32);
    return m;
}

static int usage()
{
    std::fprintf(stderr, "usage: dbow2_ref transform voc.txt desc.bin levelsup | resave in.txt out.txt | distance pairs.bin | "
                         "randomint seed d0 d1 ...\n");
    return 64;
}

int main(int argc, char** argv)
{
    if (argc < 2) return usage();
    const std::string mode = argv[1];
    if (mode == "transform" && argc == 5) {
        Vocabulary voc;
        if (!voc.loadFromTextFile(argv[2])) return 2;
        std::vector<unsigned char> raw;
        if (!slurp(argv[3], raw) || raw.size() % 32) return 3;
        std::vector<cv::Mat> features;
        for (size_t i = 0; i < raw.size() / 32; i++) features.push_back(row32(&raw[i * 32]));
        DBoW2::BowVector bow;
        DBoW2::FeatureVector fv;
        voc.transform(features, bow, fv, std::atoi(argv[4]));
        std::printf("%zu %zu %u\n", bow.size(), fv.size(), voc.size());
        for (DBoW2::BowVector::const_iterator it = bow.begin(); it != bow.end(); ++it) std::printf("%u %a\n", it->first, it->second);
        for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
            std::printf("%u %zu", it->first, it->second.size());
            for (size_t j = 0; j < it->second.size(); j++) std::printf(" %u", it->second[j]);
            std::printf("\n");
        }
        return 0;
    }
    if (mode == "resave" && argc == 4) {
        Vocabulary voc;
        if (!voc.loadFromTextFile(argv[2])) return 2;
        voc.saveToTextFile(argv[3]);
        return 0;
    }
    if (mode == "distance" && argc == 3) {
        std::vector<unsigned char> raw;
        if (!slurp(argv[2], raw) || raw.size() % 64) return 3;
        for (size_t i = 0; i < raw.size() / 64; i++)
            std::printf("%d\n", DBoW2::FORB::distance(row32(&raw[i * 64]), row32(&raw[i * 64 + 32])));
        return 0;
    }
    if (mode == "randomint" && argc >= 3) {
        DUtils::Random::SeedRandOnce(std::atoi(argv[2]));
        for (int i = 3; i < argc; i++) std::printf("%d\n", DUtils::Random::RandomInt(0, std::atoi(argv[i]) - 1));
        return 0;
    }
    return usage();
}
