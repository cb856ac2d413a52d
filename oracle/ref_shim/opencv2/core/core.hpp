// Stand-in for <opencv2/core/core.hpp>, written for this project.  It is NOT OpenCV and holds no OpenCV text: it declares
// only the names that the reference's Thirdparty/DBoW2 uses, so that DBoW2 compiles into oracle/_ref/dbow2_ref on a machine
// without OpenCV (oracle/Makefile, target `ref`).
//   cv::Mat          one owned, zero-filled row-major buffer: rows, cols, data, create, zeros, ptr<T>, release, empty, clone
//   cv::FileStorage  inert (never opened) -- DBoW2's YAML load/save only has to compile; the driver uses the text format
//   cv::FileNode     inert
// The standard headers below are the ones DBoW2 relies on the real header to pull in.
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_32F 5

namespace cv {

class Mat {
public:
    int rows = 0, cols = 0;
    unsigned char* data = nullptr;

    Mat() {}
    Mat(int r, int c, int type) { create(r, c, type); }
    void create(int r, int c, int type)
    {
        rows = r;
        cols = c;
        elem_ = type == CV_32F ? 4 : 1;
        // zero-filled, so that nothing the reference reads before writing is indeterminate; 8 spare bytes behind the rows
        store_.reset(new unsigned char[bytes() + 8](), std::default_delete<unsigned char[]>());
        data = store_.get();
    }
    static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }
    template <class T> T* ptr(int row = 0) { return reinterpret_cast<T*>(data + (size_t)row * cols * elem_); }
    template <class T> const T* ptr(int row = 0) const { return reinterpret_cast<const T*>(data + (size_t)row * cols * elem_); }
    bool empty() const { return data == nullptr; }
    void release()
    {
        store_.reset();
        data = nullptr;
        rows = cols = 0;
    }
    Mat clone() const
    {
        Mat m;
        if (data) {
            m.create(rows, cols, elem_ == 4 ? CV_32F : CV_8U);
            std::memcpy(m.data, data, bytes());
        }
        return m;
    }

private:
    size_t bytes() const { return (size_t)rows * cols * elem_; }
    std::shared_ptr<unsigned char> store_;  // copies of a Mat share the buffer, as headers of the real class do
    int elem_ = 1;
};

class FileNode {
public:
    FileNode operator[](const char*) const { return FileNode(); }
    FileNode operator[](const std::string&) const { return FileNode(); }
    FileNode operator[](int) const { return FileNode(); }
    size_t size() const { return 0; }
    operator int() const { return 0; }
    operator float() const { return 0.f; }
    operator double() const { return 0.0; }
    operator std::string() const { return std::string(); }
};

class FileStorage {
public:
    enum { READ = 0, WRITE = 1 };
    FileStorage(const char*, int) {}
    FileStorage(const std::string&, int) {}
    bool isOpened() const { return false; }
    FileNode operator[](const char*) const { return FileNode(); }
    FileNode operator[](const std::string&) const { return FileNode(); }
};

template <class T> inline FileStorage& operator<<(FileStorage& fs, const T&) { return fs; }

}  // namespace cv
