// cocoa_predict -- score a LIBSVM file with a model written by
// cocoa_driver --modelDir (cocoa_model_save): loads the rows with
// cocoa_load_libsvm, computes the decision values x.w on the GPU (cocoa_score)
// and prints the classification error as the driver's summary does
// (OptUtils.computeClassificationError, OptUtils.scala:95-98).
//   --modelFile= --testFile= [--numFeatures=] [--numSplits=1] [--outFile=]
//   [--device=0] [--strict=false]
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "cocoa_capi.h"
#include "jdouble.h"

namespace {

std::string jstr(double x) { return cocoa::jdouble::to_string(x); }

void check(int rc, const cocoa_ctx* ctx = nullptr) {
    if (rc != COCOA_OK) throw std::runtime_error(cocoa_last_error(ctx));
}

int to_int(const std::string& s) {
    char* e = nullptr;
    const long long v = std::strtoll(s.c_str(), &e, 10);
    if (s.empty() || *e || v > 2147483647LL || v < -2147483648LL)
        throw std::runtime_error("NumberFormatException: For input string: \"" + s + "\"");
    return (int)v;
}

bool to_bool(const std::string& s) {
    if (s == "true" || s == "True" || s == "TRUE") return true;
    if (s == "false" || s == "False" || s == "FALSE") return false;
    throw std::runtime_error("IllegalArgumentException: For input string: \"" + s + "\"");
}

}  // namespace

int main(int argc, char** argv) {
    try {
        std::map<std::string, std::string> opt;
        for (int i = 1; i < argc; ++i) {
            std::string a = argv[i];
            size_t b = 0;
            while (b < a.size() && a[b] == '-') ++b;
            a = a.substr(b);
            const size_t q = a.find('=');
            if (q == std::string::npos) opt[a] = "true";
            else opt[a.substr(0, q)] = a.substr(q + 1);
        }
        auto get = [&](const char* k, const char* dflt) { return opt.count(k) ? opt[k] : std::string(dflt); };
        const std::string modelFile = get("modelFile", ""), testFile = get("testFile", ""), outFile = get("outFile", "");
        if (modelFile.empty() || testFile.empty())
            throw std::runtime_error("IllegalArgumentException: --modelFile= and --testFile= are required");
        const int numSplits = to_int(get("numSplits", "1"));
        const int device = to_int(get("device", "0"));
        const bool strict = to_bool(get("strict", "false"));

        double* w = nullptr;
        int32_t d = 0;
        check(cocoa_model_load(modelFile.c_str(), &w, &d));
        const int numFeatures = opt.count("numFeatures") ? to_int(opt["numFeatures"]) : d;
        if (numFeatures != d)
            throw std::runtime_error("IllegalArgumentException: --numFeatures=" + std::to_string(numFeatures) +
                                     " but the model has " + std::to_string(d) + " features");
        cocoa_dataset test{};
        check(cocoa_load_libsvm(testFile.c_str(), numSplits, numFeatures, &test));
        cocoa_ctx* ctx = nullptr;
        check(cocoa_create(device, strict ? 1 : 0, nullptr, &ctx));
        std::vector<double> f((size_t)test.n_rows);
        check(cocoa_score(ctx, w, test.row_ptr, test.col, test.val, test.n_rows, numFeatures, f.data()), ctx);
        int64_t err = 0;
        check(cocoa_score_errors(f.data(), test.y, test.n_rows, &err));
        if (!outFile.empty()) {
            FILE* o = std::fopen(outFile.c_str(), "wb");
            if (!o) throw std::runtime_error("cannot open " + outFile);
            for (double v : f) std::fprintf(o, "%s\n", jstr(v).c_str());
            if (std::fclose(o) != 0) throw std::runtime_error("cannot write " + outFile);
        }
        std::printf("rows: %lld\n", (long long)test.n_rows);
        std::printf("test error: %s\n", jstr((double)err / (double)test.n_rows).c_str());
        std::fflush(stdout);
        cocoa_destroy(ctx);
        cocoa_dataset_free(&test);
        cocoa_model_free(w);
        return 0;
    } catch (const std::exception& e) {
        std::fflush(stdout);
        std::fprintf(stderr, "Exception in thread \"main\" %s\n", e.what());
        return 1;
    }
}
