#pragma once
#include <optional>
namespace boost {
struct none_t {};
constexpr none_t none{};
template <typename T>
class optional : public std::optional<T> {
 public:
  optional() = default;
  optional(none_t) {}
  optional(const T& v) : std::optional<T>(v) {}
  optional& operator=(none_t) { this->reset(); return *this; }
  optional& operator=(const T& v) { std::optional<T>::operator=(v); return *this; }
};
}  // namespace boost
