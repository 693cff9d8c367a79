// isle_amd/host/infer_text_main.cpp — the per-document topic files by the host loops alone, the C++ yardstick of isle_hip_infer_text as
// model_text_main is the yardstick of isle_hip_model_text: reads the arrays of an inference result from a binary file and writes the bytes
// of trainer_detail::write_doc_topic_lines (trainer_hip.h) to <out>.  No device is touched.
//   infer_text_main entries <in> <rows> <number_base> <out> [reps]   <in>: int64 offs[rows + 1], uint32 topic[n], float32 weight[n], n = offs[rows]
//   infer_text_main top     <in> <rows> <number_base> <out> [reps]   <in>: int32 top_topic[5 rows], float32 top_weight[5 rows]
// With [reps] the loop runs that many times and one line "host.<kind> <median wall ms>" goes to stdout (tools/infer_text_probe.py).
#include "trainer_hip.h"

using namespace ISLE;

template <class T>
static void read_array(std::ifstream& in, std::vector<T>& v, size_t n, const char* name) {
  v.resize(n);
  in.read((char*)v.data(), (std::streamsize)(n * sizeof(T)));
  if ((size_t)in.gcount() != n * sizeof(T)) throw std::runtime_error(std::string("short read on ") + name);
}

int main(int argc, char** argv) {
  if (argc != 6 && argc != 7) {
    std::cerr << "usage: infer_text_main entries|top <in> <rows> <number_base> <out> [reps]\n";
    return 2;
  }
  const std::string kind = argv[1];
  const uint64_t rows = std::strtoull(argv[3], nullptr, 10), base = std::strtoull(argv[4], nullptr, 10);
  const int reps = argc == 7 ? atoi(argv[6]) : 0;
  try {
    std::ifstream in(argv[2], std::ios::binary);
    if (!in) throw std::runtime_error(std::string("cannot open ") + argv[2]);
    std::vector<int64_t> offs;
    std::vector<uint32_t> topic;
    std::vector<int32_t> top_topic;
    std::vector<float> weight;
    if (kind == "entries") {
      read_array(in, offs, rows + 1, "offs");
      read_array(in, topic, (size_t)offs[rows], "topic");
      read_array(in, weight, (size_t)offs[rows], "weight");
    } else if (kind == "top") {
      read_array(in, top_topic, 5 * rows, "top_topic");
      read_array(in, weight, 5 * rows, "top_weight");
    } else {
      throw std::runtime_error("unknown kind " + kind);
    }
    std::vector<double> ms;
    for (int i = 0; i < std::max(reps, 1); ++i) {
      const auto t0 = std::chrono::steady_clock::now();
      FILE* fp = std::fopen(argv[5], "wb");
      if (!fp) throw std::runtime_error(std::string("cannot open ") + argv[5]);
      if (kind == "entries") trainer_detail::write_doc_topic_lines(fp, offs.data(), topic.data(), weight.data(), rows, base);
      else trainer_detail::write_doc_topic_lines(fp, nullptr, top_topic.data(), weight.data(), rows, base);
      std::fclose(fp);
      ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    if (reps > 0) std::cout << "host." << kind << " " << ms[ms.size() / 2] << std::endl;
  } catch (const std::exception& e) {
    std::cerr << "infer_text_main failed: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
