// isle_amd/host/model_read_main.cpp — the host parser of model_read.h on a model file: the model as raw float32 (vocab x ncols,
// column-major) for comparisons, and with [reps] its wall time for tools/model_load_probe.py: the file is read once, the parse of the
// bytes in memory runs that many times and one line "host.<format> <median wall ms>" goes to stdout.  A text the parser refuses: its
// message on stderr, exit status 3.  No device is touched.
//   model_read_main <file> <vocab> <ncols> <sparse|dense> <base> <out.f32 | -> [reps]
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <iostream>

#include "model_read.h"

using namespace ISLE;

int main(int argc, char** argv) {
  if (argc != 7 && argc != 8) {
    std::cerr << "usage: model_read_main <file> <vocab> <ncols> <sparse|dense> <base> <out.f32 | -> [reps]\n";
    return 2;
  }
  const uint64_t vocab = std::strtoull(argv[2], nullptr, 10), ncols = std::strtoull(argv[3], nullptr, 10);
  const std::string format = argv[4], out = argv[6];
  const unsigned base = (unsigned)std::atoi(argv[5]);
  const int reps = argc == 8 ? std::atoi(argv[7]) : 0;
  if (format != "sparse" && format != "dense") {
    std::cerr << "model_read_main: format is sparse or dense\n";
    return 2;
  }
  try {
    const std::vector<char> text = model_read::read_file(argv[1]);
    std::vector<float> model, by_word;
    std::vector<double> ms;
    for (int i = 0; i < std::max(reps, 1); ++i) {
      const auto t0 = std::chrono::steady_clock::now();
      if (format == "sparse") model_read::read_sparse_model(text.data(), text.size(), ncols, vocab, base, by_word, nullptr);
      else model_read::read_dense_model(text.data(), text.size(), ncols, vocab, model);
      ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    if (reps > 0) std::cout << "host." << format << " " << ms[ms.size() / 2] << std::endl;
    if (out != "-") {
      if (format == "sparse") {  // word-major -> column-major
        model.resize(vocab * ncols);
        for (uint64_t w = 0; w < vocab; ++w)
          for (uint64_t t = 0; t < ncols; ++t) model[w + t * vocab] = by_word[w * ncols + t];
      }
      std::ofstream f(out, std::ios::binary);
      f.write((const char*)model.data(), (std::streamsize)(model.size() * sizeof(float)));
      if (!f) throw std::runtime_error("cannot write " + out);
    }
  } catch (const std::exception& e) {
    std::cerr << "model_read_main: " << e.what() << std::endl;
    return 3;
  }
  return 0;
}
