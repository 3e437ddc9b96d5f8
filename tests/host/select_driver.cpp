// select_driver.cpp -- HIPDetector<bool> with keepStrongest(true) on a frame that overflows opts.maxkp, driven through the policy host
// the way ColoC drives GPUDetector (reference FeatureDetector.hpp:21-32), then switched back to the default rule on the same
// detector.  Dumps keypoints, regions and the uncapped count as raw files for tests/test_gpu_detect_select.py.
// usage: select_driver <dir> <width> <height> <maxkp>     (reads <dir>/img0.pgm)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "HIPDetector.hpp"

template <typename T, template <class> class ProcessorType>
class FeatureDetector : public ProcessorType<T> {   // policy host, reference FeatureDetector.hpp:21-32
public:
    explicit FeatureDetector(coloc::DetectorOptions& opts) : ProcessorType<T>(opts) {}
    T detectFeaturesFile(unsigned int idx, coloc::FeatureMap& regions, std::string& imageName)
    {
        return ProcessorType<T>::detectFeaturesFile(idx, regions, imageName);
    }
};

static void dump(const std::string& path, const void* p, size_t bytes)
{
    std::ofstream f(path, std::ios::binary);
    f.write(static_cast<const char*>(p), static_cast<std::streamsize>(bytes));
}

int main(int argc, char** argv)
{
    if (argc < 5) { std::fprintf(stderr, "usage: %s dir width height maxkp\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    coloc::DetectorOptions dopts{ 1.2f, 8, static_cast<unsigned>(std::atoi(argv[2])), static_cast<unsigned>(std::atoi(argv[3])),
                                  static_cast<unsigned>(std::atoi(argv[4])), 40 };
    FeatureDetector<bool, coloc::HIPDetector> detector(dopts);
    std::string name = dir + "/img0.pgm";
    const char* tags[3] = { "strongest", "first", "again" };
    for (int pass = 0; pass < 3; ++pass) {
        detector.keepStrongest(pass != 1);
        coloc::FeatureMap regions;
        if (detector.detectFeaturesFile(0, regions, name) != EXIT_SUCCESS) { std::fprintf(stderr, "detect failed: %s\n", detector.lastError()); return 1; }
        const std::string t = tags[pass];
        dump(dir + "/kps_" + t + ".bin", detector.kps.data(), detector.kps.size() * sizeof(Keypoint));
        dump(dir + "/desc_" + t + ".bin", regions[0]->DescriptorRawData(), regions[0]->RegionCount() * 64);
        dump(dir + "/feat_" + t + ".bin", regions[0]->Features().data(), regions[0]->RegionCount() * 16);
        const int found = detector.keypointsFound();
        dump(dir + "/found_" + t + ".bin", &found, sizeof found);
    }
    std::printf("ok\n");
    return 0;
}
